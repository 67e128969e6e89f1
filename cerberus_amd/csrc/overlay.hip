// Instance overlays drawn on the device (include/cerberus_hip.h, section "instance overlays"; cerberus_amd/viz.py): closed contours rasterised as
// round-capped, round-jointed strokes into a priority plane, then one resolve pass that colours the picture and up-scales its source.
//
// The DEFINITION is the header's and is all integers.  A pixel (x, y) is covered by the segment a -> b drawn with width w (1..255) iff the distance
// from its centre to the segment is at most w / 2.  With v = b - a, u = p - a, vv = v.v, t = u.v, c = ux vy - uy vx:
//     vv == 0 or t <= 0 :  4 (u.u)     <= w^2                (the disk round a)
//     t >= vv           :  4 |p - b|^2 <= w^2                (the disk round b)
//     otherwise         :  |c| <= isqrt(floor(w^2 vv / 4))   (the band; c is an integer, so this is c^2 <= w^2 vv / 4 exactly)
// isqrt is taken once per segment (a double square root corrected by integer checks).  Coordinates are at most 2^20 in magnitude and pixels lie inside
// an image of at most 32768 a side: |u|, |v| < 2^22, every product fits 2^45 and w^2 vv < 2^61 -- nothing overflows int64.  An even width paints
// w + 1 pixels across an axis-aligned line (|c| <= w / 2 holds for w + 1 integers), an odd width w.
//
//   ov_stamp_kernel    One wave per 64 contours.  The lanes load the 64 point counts and take their inclusive prefix sum by shuffles; segment s of the
//                      group belongs to the contour j with incl[j - 1] <= s < incl[j] (six shuffle steps of a binary search), so the lanes walk the
//                      group's segments 64 at a time whatever the contours' sizes.  Pass 1 transforms every point (q = p mul - org in int64, q / div
//                      truncated toward zero) and marks the contours that have a coordinate outside [-2^20, 2^20]: such a contour is skipped as a whole.
//                      Pass 2 draws.  Every segment's box is expanded by (w + 1) / 2 and clipped to the image, which bounds every loop by the image
//                      size.  A box of at most OV_SMALL pixels (a nucleus edge) is walked by its own lane; the larger ones of the 64 in flight are
//                      taken one after the other by the whole wave (ballot + shuffle broadcast): row by row, the row narrowed to the x-interval the
//                      stroke can reach -- the piece of the segment whose y lies within (w + 1) / 2 of the row, widened by the same amount -- and the
//                      lanes stride over that interval; where the interval is narrower than the wave (steep segments) the 64 lanes form
//                      LR rows x LW columns and take LR rows per step.  The predicate alone decides what is painted; the traversal only has to
//                      offer a superset.  A long segment still belongs to ONE wave (a 2000-px edge: a few hundred steps).
//                      A call with few groups (a tile's dozen glands of a thousand points each) gives every group up to 64 waves (gridDim.y):
//                      each runs pass 1 in full and takes every gridDim.y-th batch of 64 segments.
//                      Painter's order without order: a covered pixel takes max(plane, ordinal) with an integer atomic max.
//   ov_resolve_kernel  dst = colour[prio - 1] where the plane is non-zero (and names a colour), else src[y / up][x / up].  One thread per output pixel,
//                      three byte stores: rows may start at any byte (row strides in bytes, padded rows), and the pass moves 7 bytes per pixel.
//   ov_fill_kernel     The INTERIOR of the same contours into the same plane (the header's "label maps from contours": even-odd on pixel centres, the
//                      ray pointing left, rows half-open).  Same groups, same pass 1 (ov_pass1) -- which here also takes every contour's box of
//                      transformed points (LDS min / max).  The interior of a contour lies in columns xmin .. xmax - 1 and rows ymin .. ymax - 1 (at
//                      x = xmax every crossing of the row counts, and a closed polygon crosses a row an even number of times); that box, clipped to
//                      the image, is cut into 64 x 64 cells and the group's (contour, cell) items are dealt round-robin to the gridDim.y waves
//                      that share the group.  Lane r of a wave owns row y0 + r of the cell as a 64-bit mask in a register.  The wave walks the
//                      contour's edges 64 at a time: a lane loads one edge and says whether it can matter to this cell (crosses one of its rows,
//                      not wholly to its right); the ones that do are broadcast one after the other (ballot + shuffle) and every lane whose row
//                      the edge crosses XORs ~0 << clamp(xc - x0, 0, 64) into its mask -- no LDS and no atomic while accumulating.  xc is the exact
//                      integer ceiling (a double quotient corrected by integer checks, as ov_isqrt).  Writing: the row masks are broadcast one at
//                      a time and lane c issues the atomic max for column c, so that one atomic instruction covers one contiguous row segment.
//                      Every loop is bounded by the clipped box; a wave's time grows with points x cells.
//   ov_labels_kernel   dst = table[prio - 1] where the plane is non-zero (and names an entry), else `background`: int32, one thread per pixel, 8 bytes
//                      per pixel.
// Plain vector loads / stores and integer atomics only; no LDS apart from a wave's 64 skip flags (and, in the fill, its 64 boxes); all pixel offsets
// are 64-bit.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <string>

#include "../../include/cerberus_hip.h"

int cerb_set_error(const std::string& m);  // cerb_api.hip
#define OV_OK(expr)                                                                                   \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return cerb_set_error(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace {

typedef long long i64;
constexpr int OV_MAX_SIDE = 32768;
constexpr int OV_SMALL = 64;            // clipped boxes of at most this many pixels are walked by one lane
constexpr i64 OV_COORD = 1ll << 20;     // a contour with a transformed coordinate beyond +-this is skipped
constexpr i64 OV_FILL_WAVES = 2048;     // a stamp call is spread over about this many waves (256 CUs x 8) when it has fewer contour groups
constexpr i64 OV_MAX_TOTAL = 0xFFFFFFFFll - 1;  // ordinals are 1 .. 2^32 - 2

struct OvSeg {
    int ax, ay, vx, vy;
    i64 vv, thr;
    int w2;
};

__device__ __forceinline__ i64 ov_isqrt(i64 x) {  // exact floor(sqrt(x)), 0 <= x < 2^62
    i64 r = (i64)sqrt((double)x);
    while (r * r > x) --r;
    while ((r + 1) * (r + 1) <= x) ++r;
    return r;
}

__device__ __forceinline__ OvSeg ov_make(int ax, int ay, int bx, int by, int w) {
    OvSeg s;
    s.ax = ax, s.ay = ay, s.vx = bx - ax, s.vy = by - ay;
    s.vv = (i64)s.vx * s.vx + (i64)s.vy * s.vy;
    s.w2 = w * w;
    s.thr = ov_isqrt(((i64)s.w2 * s.vv) >> 2);
    return s;
}

__device__ __forceinline__ bool ov_covered(const OvSeg& s, int px, int py) {
    const i64 ux = px - s.ax, uy = py - s.ay;
    const i64 t = ux * s.vx + uy * s.vy;
    if (s.vv == 0 || t <= 0) return 4 * (ux * ux + uy * uy) <= s.w2;
    if (t >= s.vv) {
        const i64 dx = ux - s.vx, dy = uy - s.vy;
        return 4 * (dx * dx + dy * dy) <= s.w2;
    }
    const i64 c = ux * s.vy - uy * s.vx;
    return (c < 0 ? -c : c) <= s.thr;
}

__device__ __forceinline__ i64 ov_floor_div(i64 a, i64 b) {  // b != 0
    const i64 q = a / b;
    return ((a % b != 0) && ((a < 0) != (b < 0))) ? q - 1 : q;
}

// point k of a contour after the call's transform; false when a coordinate leaves the range
__device__ __forceinline__ bool ov_point(const int32_t* __restrict__ pts, i64 idx, int mul, int div, i64 org_x, i64 org_y, int& x, int& y) {
    const i64 qx = (i64)pts[2 * idx] * mul - org_x, qy = (i64)pts[2 * idx + 1] * mul - org_y;
    const i64 tx = qx / div, ty = qy / div;  // C: toward zero
    x = (int)tx, y = (int)ty;
    return tx >= -OV_COORD && tx <= OV_COORD && ty >= -OV_COORD && ty <= OV_COORD;
}

// segment s of a 64-contour group -> (contour j inside the group, segment k of it); incl: this lane's inclusive prefix sum.  Every lane calls it.
__device__ __forceinline__ void ov_locate(i64 incl, i64 s, int& j, i64& k) {
    int lo = 0, hi = 63;
#pragma unroll
    for (int it = 0; it < 6; ++it) {
        const int mid = (lo + hi) >> 1;
        const i64 v = __shfl(incl, mid);
        if (v > s) hi = mid;
        else lo = mid + 1;
    }
    j = lo;
    const i64 before = __shfl(incl, j > 0 ? j - 1 : 0);
    k = s - (j > 0 ? before : 0);
}

// inclusive prefix sum of v over the 64 lanes of the wave
__device__ __forceinline__ i64 ov_incl(i64 v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const i64 a = __shfl_up(v, d);
        if (lane >= d) v += a;
    }
    return v;
}

// Pass 1 of a 64-contour group: every point through the call's transform, 64 at a time whatever the contours' sizes; bad[j] = 1 for a contour with a
// coordinate outside the range (every writer stores the same word).  BOX: box[j] = (xmin, xmax, ymin, ymax) of contour j's transformed points as well
// (preset by the caller; meaningless for a contour marked bad).  Every lane calls it; the caller synchronises before and after.
template <bool BOX>
__device__ __forceinline__ void ov_pass1(const int32_t* __restrict__ pts, i64 incl_p, i64 tot_p, i64 off, int lane, int mul, int div, i64 org_x, i64 org_y,
                                         uint32_t* bad, int (*box)[4]) {
    for (i64 b0 = 0; b0 < tot_p; b0 += 64) {
        const i64 s = b0 + lane;
        int j;
        i64 k;
        ov_locate(incl_p, s < tot_p ? s : tot_p - 1, j, k);
        const i64 joff = __shfl(off, j);
        if (s < tot_p) {
            int x, y;
            if (!ov_point(pts, joff + k, mul, div, org_x, org_y, x, y)) bad[j] = 1;
            else if (BOX) atomicMin(&box[j][0], x), atomicMax(&box[j][1], x), atomicMin(&box[j][2], y), atomicMax(&box[j][3], y);
        }
    }
}

__global__ __launch_bounds__(64) void ov_stamp_kernel(const int32_t* __restrict__ pts, const i64* __restrict__ offsets, const int32_t* __restrict__ counts,
                                                      i64 n, int mul, int div, i64 org_x, i64 org_y, int width, uint32_t first_ordinal,
                                                      uint32_t* __restrict__ plane, int H, int W) {
    __shared__ uint32_t bad[64];
    const int lane = threadIdx.x;
    const i64 base_c = (i64)blockIdx.x * 64;
    const i64 ci = base_c + lane;
    const int cnt = ci < n ? counts[ci] : 0;
    const i64 off = ci < n ? offsets[ci] : 0;
    // points read in pass 1: all of them; segments drawn in pass 2: a count of 2 is ONE capsule (its closing segment is the same set)
    const i64 npt = cnt > 0 ? cnt : 0;
    const i64 nseg = cnt == 2 ? 1 : npt;
    const i64 incl_p = ov_incl(npt, lane), incl_s = ov_incl(nseg, lane);
    const i64 tot_p = __shfl(incl_p, 63), tot_s = __shfl(incl_s, 63);
    if (tot_p == 0) return;  // (uniform over the wave)
    bad[lane] = 0;
    __syncthreads();
    ov_pass1<false>(pts, incl_p, tot_p, off, lane, mul, div, org_x, org_y, bad, nullptr);
    __syncthreads();
    const uint32_t my_bad = bad[lane];
    const int e = (width + 1) >> 1;
    // the group's segments in batches of 64, dealt round-robin to the gridDim.y waves that share the group (each of them has run pass 1 in full)
    for (i64 b0 = (i64)blockIdx.y * 64; b0 < tot_s; b0 += 64ll * gridDim.y) {
        const i64 s = b0 + lane;
        int j;
        i64 k;
        ov_locate(incl_s, s < tot_s ? s : tot_s - 1, j, k);
        const i64 joff = __shfl(off, j);
        const int jcnt = __shfl(cnt, j);
        const uint32_t jbad = __shfl(my_bad, j);
        int ax = 0, ay = 0, bx = 0, by = 0, x0 = 0, x1 = -1, y0 = 0, y1 = -1;
        const uint32_t ord = first_ordinal + (uint32_t)(base_c + j) + 1u;
        if (s < tot_s && !jbad) {
            const i64 k2 = k + 1 < jcnt ? k + 1 : 0;
            ov_point(pts, joff + k, mul, div, org_x, org_y, ax, ay);
            ov_point(pts, joff + k2, mul, div, org_x, org_y, bx, by);
            x0 = (ax < bx ? ax : bx) - e, x1 = (ax > bx ? ax : bx) + e;
            y0 = (ay < by ? ay : by) - e, y1 = (ay > by ? ay : by) + e;
            x0 = x0 < 0 ? 0 : x0, y0 = y0 < 0 ? 0 : y0;
            x1 = x1 > W - 1 ? W - 1 : x1, y1 = y1 > H - 1 ? H - 1 : y1;
        }
        const bool live = x0 <= x1 && y0 <= y1;
        const i64 area = live ? (i64)(x1 - x0 + 1) * (y1 - y0 + 1) : 0;
        if (live && area <= OV_SMALL) {
            const OvSeg sg = ov_make(ax, ay, bx, by, width);
            for (int y = y0; y <= y1; ++y)
                for (int x = x0; x <= x1; ++x)
                    if (ov_covered(sg, x, y)) atomicMax(&plane[(size_t)y * W + x], ord);
        }
        unsigned long long big = __ballot(live && area > OV_SMALL);
        while (big) {  // (uniform over the wave)
            const int src = __ffsll((long long)big) - 1;
            big &= big - 1;
            const int sax = __shfl(ax, src), say = __shfl(ay, src), sbx = __shfl(bx, src), sby = __shfl(by, src);
            const int sx0 = __shfl(x0, src), sx1 = __shfl(x1, src), sy0 = __shfl(y0, src), sy1 = __shfl(y1, src);
            const uint32_t sord = __shfl(ord, src);
            const OvSeg sg = ov_make(sax, say, sbx, sby, width);
            const int ymin = say < sby ? say : sby, ymax = say > sby ? say : sby;
            // lanes as LR rows x LW columns: LW = the power of two (4..64) that covers a row's interval -- a vertical 12-px stroke takes 4 rows per
            // step instead of 1 with 13 of 64 lanes at work.  (An estimate: it only decides how the candidates are shared out.)
            i64 wd = (i64)sx1 - sx0 + 1;
            if (sg.vy != 0) {
                const i64 avx = sg.vx < 0 ? -(i64)sg.vx : sg.vx, avy = sg.vy < 0 ? -(i64)sg.vy : sg.vy;
                const i64 est = avx * (2 * e) / avy + 2 * e + 2;
                wd = est < wd ? est : wd;
            }
            int lw_log = 6;
            while (lw_log > 2 && (1ll << (lw_log - 1)) >= wd) --lw_log;
            const int LW = 1 << lw_log, LR = 64 >> lw_log, lr = lane >> lw_log, lc = lane & (LW - 1);
            for (int yb = sy0; yb <= sy1; yb += LR) {
                const int y = yb + lr;
                if (y > sy1) continue;
                int xa = sx0, xb = sx1;
                if (sg.vy != 0) {
                    // the stroke's pixels of this row lie within e of the piece of the segment whose y is in [y - e, y + e] (clamped to the segment)
                    int ylo = y - e, yhi = y + e;
                    ylo = ylo < ymin ? ymin : (ylo > ymax ? ymax : ylo);
                    yhi = yhi < ymin ? ymin : (yhi > ymax ? ymax : yhi);
                    const i64 n0 = (i64)(ylo - say) * sg.vx, n1 = (i64)(yhi - say) * sg.vx;
                    const i64 f0 = ov_floor_div(n0, sg.vy), f1 = ov_floor_div(n1, sg.vy);
                    const i64 lo = (f0 < f1 ? f0 : f1) + sax - e, hi = (f0 > f1 ? f0 : f1) + 1 + sax + e;
                    xa = lo > xa ? (int)lo : xa;
                    xb = hi < xb ? (int)hi : xb;
                }
                for (int x = xa + lc; x <= xb; x += LW)
                    if (ov_covered(sg, x, y)) atomicMax(&plane[(size_t)y * W + x], sord);
            }
        }
    }
}

// exact ceil(num / den), den > 0, |num| < 2^44 and |num / den| < 2^22: a double quotient (off by far less than 1) corrected by integer checks
__device__ __forceinline__ i64 ov_ceil_div(i64 num, i64 den) {
    i64 c = (i64)ceil((double)num / (double)den);
    while ((c - 1) * den >= num) --c;
    while (c * den < num) ++c;
    return c;
}

__global__ __launch_bounds__(64) void ov_fill_kernel(const int32_t* __restrict__ pts, const i64* __restrict__ offsets, const int32_t* __restrict__ counts,
                                                     i64 n, int mul, int div, i64 org_x, i64 org_y, uint32_t first_ordinal, uint32_t* __restrict__ plane,
                                                     int H, int W) {
    __shared__ uint32_t bad[64];
    __shared__ int box[64][4];
    const int lane = threadIdx.x;
    const i64 base_c = (i64)blockIdx.x * 64;
    const i64 ci = base_c + lane;
    const int cnt = ci < n ? counts[ci] : 0;
    const i64 off = ci < n ? offsets[ci] : 0;
    const i64 incl_p = ov_incl(cnt > 0 ? cnt : 0, lane);
    const i64 tot_p = __shfl(incl_p, 63);
    if (tot_p == 0) return;  // (uniform over the wave)
    bad[lane] = 0;
    box[lane][0] = box[lane][2] = INT_MAX, box[lane][1] = box[lane][3] = INT_MIN;
    __syncthreads();
    ov_pass1<true>(pts, incl_p, tot_p, off, lane, mul, div, org_x, org_y, bad, box);
    __syncthreads();
    // this lane's contour: the clipped box of its interior and the cells it is cut into (fewer than 3 points, skipped, flat or outside: none)
    int fx0 = 0, fx1 = -1, fy0 = 0, fy1 = -1, ncx = 0, ncy = 0;
    if (cnt >= 3 && !bad[lane]) {
        fx0 = box[lane][0] < 0 ? 0 : box[lane][0], fx1 = box[lane][1] - 1 > W - 1 ? W - 1 : box[lane][1] - 1;
        fy0 = box[lane][2] < 0 ? 0 : box[lane][2], fy1 = box[lane][3] - 1 > H - 1 ? H - 1 : box[lane][3] - 1;
        if (fx0 <= fx1 && fy0 <= fy1) ncx = ((fx1 - fx0) >> 6) + 1, ncy = ((fy1 - fy0) >> 6) + 1;
    }
    const i64 incl_i = ov_incl((i64)ncx * ncy, lane);
    const i64 tot_i = __shfl(incl_i, 63);
    // the group's (contour, cell) items, dealt round-robin to the gridDim.y waves that share the group (each of them has run pass 1 in full)
    for (i64 t = blockIdx.y; t < tot_i; t += gridDim.y) {
        int j;
        i64 k;
        ov_locate(incl_i, t, j, k);
        const i64 joff = __shfl(off, j);
        const int jcnt = __shfl(cnt, j), jncx = __shfl(ncx, j);
        const int jx0 = __shfl(fx0, j), jx1 = __shfl(fx1, j), jy0 = __shfl(fy0, j), jy1 = __shfl(fy1, j);
        const int x0 = jx0 + (int)(k % jncx) * 64, y0 = jy0 + (int)(k / jncx) * 64;  // the cell's first column and row
        const int ylast = y0 + 63 < jy1 ? y0 + 63 : jy1;
        const int y = y0 + lane;  // this lane's row (rows past ylast are accumulated and never written)
        unsigned long long mask = 0;
        for (int e0 = 0; e0 < jcnt; e0 += 64) {
            const int e = e0 + lane;
            int ax = 0, ay = 0;
            if (e < jcnt) ov_point(pts, joff + e, mul, div, org_x, org_y, ax, ay);
            int bx = __shfl_down(ax, 1), by = __shfl_down(ay, 1);  // the next lane's point is this edge's end, except for lane 63 and the closing edge
            bool rel = false;
            if (e < jcnt) {
                if (lane == 63 || e + 1 == jcnt) ov_point(pts, joff + (e + 1 < jcnt ? e + 1 : 0), mul, div, org_x, org_y, bx, by);
                if (ay > by) {  // (xc does not depend on the edge's direction)
                    const int tx = ax, ty = ay;
                    ax = bx, ay = by, bx = tx, by = ty;
                }
                // it can matter to this cell: crosses one of its rows (half-open: a horizontal edge crosses none) and is not wholly to its right
                rel = ay < by && ay <= ylast && by > y0 && (ax < x0 + 64 || bx < x0 + 64);
            }
            unsigned long long todo = __ballot(rel);
            while (todo) {  // (uniform over the wave)
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int sax = __shfl(ax, src), say = __shfl(ay, src), sbx = __shfl(bx, src), sby = __shfl(by, src);
                if (y >= say && y < sby) {
                    i64 d = 0;  // wholly left of the cell: the whole row toggles
                    if (sax > x0 || sbx > x0) d = sax + ov_ceil_div((i64)(y - say) * (sbx - sax), sby - say) - x0;
                    if (d < 64) mask ^= ~0ull << (d < 0 ? 0 : d);
                }
            }
        }
        const int ncol = jx1 - x0 + 1;  // >= 1; columns past the clipped box are never written
        if (ncol < 64) mask &= (1ull << ncol) - 1;
        const uint32_t ord = first_ordinal + (uint32_t)(base_c + j) + 1u;
        for (int r = 0; r <= ylast - y0; ++r) {
            const unsigned long long m = (unsigned long long)__shfl((i64)mask, r);
            if ((m >> lane) & 1) atomicMax(&plane[(size_t)(y0 + r) * W + x0 + lane], ord);
        }
    }
}

__global__ __launch_bounds__(256) void ov_labels_kernel(const int32_t* __restrict__ table, uint32_t n_total, int32_t background, const uint32_t* __restrict__ plane,
                                                        uint8_t* __restrict__ dst, i64 dst_stride, int H, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const uint32_t pr = plane[(size_t)y * W + x];
    ((int32_t*)(dst + (i64)y * dst_stride))[x] = (pr != 0 && pr <= n_total) ? table[pr - 1] : background;
}

__global__ __launch_bounds__(256) void ov_resolve_kernel(const uint8_t* __restrict__ src, i64 src_stride, int up, const uint32_t* __restrict__ colours,
                                                         uint32_t n_total, const uint32_t* __restrict__ plane, uint8_t* __restrict__ dst, i64 dst_stride,
                                                         int H, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const uint32_t pr = plane[(size_t)y * W + x];
    uint32_t r, g, b;
    if (pr != 0 && pr <= n_total) {
        const uint32_t c = colours[pr - 1];
        r = c & 255u, g = (c >> 8) & 255u, b = (c >> 16) & 255u;
    } else {
        const uint8_t* p = src + (i64)(y / up) * src_stride + (i64)(x / up) * 3;
        r = p[0], g = p[1], b = p[2];
    }
    uint8_t* q = dst + (i64)y * dst_stride + (i64)x * 3;
    q[0] = (uint8_t)r, q[1] = (uint8_t)g, q[2] = (uint8_t)b;
}

inline bool ov_bad_size(int h, int w) { return h <= 0 || w <= 0 || h > OV_MAX_SIDE || w > OV_MAX_SIDE; }

}  // namespace

extern "C" size_t cerb_overlay_workspace_bytes(int out_h, int out_w) {
    if (ov_bad_size(out_h, out_w)) return 0;
    return (size_t)out_h * (size_t)out_w * sizeof(uint32_t);
}

extern "C" int cerb_overlay_clear(void* ws, size_t ws_bytes, int out_h, int out_w, void* hip_stream) {
    if (!ws || ov_bad_size(out_h, out_w) || ((uintptr_t)ws & 3) != 0) return cerb_set_error("cerb_overlay_clear: bad arguments");
    if (ws_bytes < cerb_overlay_workspace_bytes(out_h, out_w)) return cerb_set_error("cerb_overlay_clear: workspace too small");
    OV_OK(hipMemsetAsync(ws, 0, cerb_overlay_workspace_bytes(out_h, out_w), (hipStream_t)hip_stream));
    return 0;
}

// the checks the two calls that take contours share; `who` names the call in the message
static int ov_check_contours(const char* who, const void* points, const void* offsets, const void* counts, const void* ws, long long n, int mul, int div,
                             long long org_x, long long org_y, long long first_ordinal, size_t ws_bytes, int out_h, int out_w) {
    const std::string w(who);
    if (!points || !offsets || !counts || !ws || ((uintptr_t)ws & 3) != 0) return cerb_set_error(w + ": null or misaligned pointer");
    if (ov_bad_size(out_h, out_w)) return cerb_set_error(w + ": image sides must be 1..32768");
    if (n < 0 || first_ordinal < 0 || first_ordinal > OV_MAX_TOTAL || n > OV_MAX_TOTAL - first_ordinal)
        return cerb_set_error(w + ": n / first_ordinal negative, or 2^32 - 1 contours and more in total");
    if (mul < 1 || mul > 16 || div < 1 || div > 4096) return cerb_set_error(w + ": mul (1..16) or div (1..4096) out of range");
    if (org_x < -(1ll << 40) || org_x > (1ll << 40) || org_y < -(1ll << 40) || org_y > (1ll << 40)) return cerb_set_error(w + ": origin beyond +-2^40");
    if (ws_bytes < cerb_overlay_workspace_bytes(out_h, out_w)) return cerb_set_error(w + ": workspace too small");
    return 0;
}

extern "C" int cerb_overlay_stamp(const int32_t* points, const int64_t* offsets, const int32_t* counts, long long n, int mul, int div, long long org_x,
                                  long long org_y, int width, long long first_ordinal, void* ws, size_t ws_bytes, int out_h, int out_w, void* hip_stream) {
    if (width < 1 || width > 255) return cerb_set_error("cerb_overlay_stamp: width (1..255) out of range");
    if (int rc = ov_check_contours("cerb_overlay_stamp", points, offsets, counts, ws, n, mul, div, org_x, org_y, first_ordinal, ws_bytes, out_h, out_w)) return rc;
    if (n == 0) return 0;
    const long long blocks = (n + 63) / 64;  // < 2^26
    // few contours (a tile: a dozen glands of a thousand points each) would leave the chip to one wave per 64 of them: such calls give every group
    // up to 64 waves, which share its segment batches; a slide's 10^4 groups get one wave each
    const long long split = blocks >= OV_FILL_WAVES ? 1 : (OV_FILL_WAVES / blocks > 64 ? 64 : OV_FILL_WAVES / blocks);
    hipLaunchKernelGGL(ov_stamp_kernel, dim3((unsigned)blocks, (unsigned)split), dim3(64), 0, (hipStream_t)hip_stream, points, (const i64*)offsets, counts, (i64)n, mul, div,
                       (i64)org_x, (i64)org_y, width, (uint32_t)first_ordinal, (uint32_t*)ws, out_h, out_w);
    OV_OK(hipGetLastError());
    return 0;
}

extern "C" int cerb_overlay_resolve(const uint8_t* src, long long src_row_stride, int src_h, int src_w, int up, const uint32_t* colours, long long n_total,
                                    const void* ws, size_t ws_bytes, uint8_t* dst, long long dst_row_stride, int out_h, int out_w, void* hip_stream) {
    if (!src || !ws || !dst || ((uintptr_t)ws & 3) != 0 || ((uintptr_t)colours & 3) != 0) return cerb_set_error("cerb_overlay_resolve: null or misaligned pointer");
    if (n_total < 0 || n_total > OV_MAX_TOTAL || (n_total > 0 && !colours)) return cerb_set_error("cerb_overlay_resolve: n_total negative, 2^32 - 1 and above, or without colours");
    if (up < 1 || up > 8) return cerb_set_error("cerb_overlay_resolve: up must be 1..8");
    if (ov_bad_size(out_h, out_w) || ov_bad_size(src_h, src_w) || (long long)src_h * up != out_h || (long long)src_w * up != out_w)
        return cerb_set_error("cerb_overlay_resolve: sides must be 1..32768 with out = src * up");
    if (src_row_stride < 3ll * src_w || dst_row_stride < 3ll * out_w) return cerb_set_error("cerb_overlay_resolve: a row stride is shorter than its row");
    if (ws_bytes < cerb_overlay_workspace_bytes(out_h, out_w)) return cerb_set_error("cerb_overlay_resolve: workspace too small");
    hipLaunchKernelGGL(ov_resolve_kernel, dim3((out_w + 255) / 256, out_h), dim3(256), 0, (hipStream_t)hip_stream, src, (i64)src_row_stride, up, colours,
                       (uint32_t)n_total, (const uint32_t*)ws, dst, (i64)dst_row_stride, out_h, out_w);
    OV_OK(hipGetLastError());
    return 0;
}

extern "C" int cerb_overlay_fill(const int32_t* points, const int64_t* offsets, const int32_t* counts, long long n, int mul, int div, long long org_x,
                                 long long org_y, long long first_ordinal, void* ws, size_t ws_bytes, int out_h, int out_w, void* hip_stream) {
    if (int rc = ov_check_contours("cerb_overlay_fill", points, offsets, counts, ws, n, mul, div, org_x, org_y, first_ordinal, ws_bytes, out_h, out_w)) return rc;
    if (n == 0) return 0;
    const long long blocks = (n + 63) / 64;  // < 2^26
    // as the stamp: a call with few groups (a tile's dozen glands, each a box of many cells) gives every group up to 64 waves, which share its items
    const long long split = blocks >= OV_FILL_WAVES ? 1 : (OV_FILL_WAVES / blocks > 64 ? 64 : OV_FILL_WAVES / blocks);
    hipLaunchKernelGGL(ov_fill_kernel, dim3((unsigned)blocks, (unsigned)split), dim3(64), 0, (hipStream_t)hip_stream, points, (const i64*)offsets, counts, (i64)n, mul, div,
                       (i64)org_x, (i64)org_y, (uint32_t)first_ordinal, (uint32_t*)ws, out_h, out_w);
    OV_OK(hipGetLastError());
    return 0;
}

extern "C" int cerb_overlay_labels(const int32_t* table, long long n_total, int background, const void* ws, size_t ws_bytes, int32_t* dst,
                                   long long dst_row_stride, int out_h, int out_w, void* hip_stream) {
    if (!ws || !dst || ((uintptr_t)ws & 3) != 0 || ((uintptr_t)table & 3) != 0 || ((uintptr_t)dst & 3) != 0)
        return cerb_set_error("cerb_overlay_labels: null or misaligned pointer");
    if (n_total < 0 || n_total > OV_MAX_TOTAL || (n_total > 0 && !table)) return cerb_set_error("cerb_overlay_labels: n_total negative, 2^32 - 1 and above, or without a table");
    if (ov_bad_size(out_h, out_w)) return cerb_set_error("cerb_overlay_labels: image sides must be 1..32768");
    if (dst_row_stride < 4ll * out_w || (dst_row_stride & 3) != 0) return cerb_set_error("cerb_overlay_labels: the row stride is shorter than its row or no multiple of 4");
    if (ws_bytes < cerb_overlay_workspace_bytes(out_h, out_w)) return cerb_set_error("cerb_overlay_labels: workspace too small");
    hipLaunchKernelGGL(ov_labels_kernel, dim3((out_w + 255) / 256, out_h), dim3(256), 0, (hipStream_t)hip_stream, table, (uint32_t)n_total, (int32_t)background,
                       (const uint32_t*)ws, (uint8_t*)dst, (i64)dst_row_stride, out_h, out_w);
    OV_OK(hipGetLastError());
    return 0;
}
