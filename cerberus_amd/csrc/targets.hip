// Training targets on the device: gen_targets of the reference (loader/targets.py:185-244, loader/augs.py:7-21) from instance annotations.
//
// One "image" below is one (sample n, eroded head hd) pair, e = hd * N + n; every kernel runs over all E = heads x N images in one launch
// (blockIdx.y = e).  Planes of the workspace, all [E][H * W]:
//   ids  int32  the annotation channel of the head; after the morphology pass the inner map (0 / 1)
//   lab  int32  union-find parents / after a flatten the component root (smallest raster index of the component), -1 = background
//   flag uint8  flag[root] = 1: the component has a pixel inside the centre crop ("listed", loader/targets.py:77-79)
//   box  int32 x 4 per pixel, used at component roots only: rmin, rmax, cmin, cmax (inclusive) of an inner-map label
//
// Pipeline (cerb_target_eroded_maps):   ids -> same-id components (fix_mirror_padding's partition) -> listed flags -> inner / contour by
// the rule "every in-image pixel under the element carries one listed instance" / "some listed instance under the element" -> class map.
// (cerb_target_eroded_maps goes on:)    inner map -> components (scipy.ndimage.label's partition) -> boxes -> label count and window area.
// (cerb_target_weight_maps, after the host has sized the window workspace): per label the column pass of an exact Euclidean distance
// transform over its window (bounding box grown by the decay margin) into a uint16 plane of vertical distances; then one gather per crop
// pixel: for every label whose window covers the pixel the row pass (a search outwards from the pixel's column that stops when the
// column offset alone exceeds the best squared distance found), the two smallest squared distances over labels, and the weight.
// Squared distances are integers, the two-smallest reduction is a per-pixel gather over the label list: no float atomics, no order
// dependence -- the label list's ORDER (atomic slot counters) changes between runs, the multiset each pixel reduces does not.
//
// Why not pp_label.hip's labeller: its predicate is a byte plane compared with one value and it labels ONE map per call with tile-local
// LDS passes tuned for slide-sized maps; here the predicate is "equal non-zero id", the maps are a few hundred pixels on a side and there
// are N x heads of them per call.  The union-find itself (atomicMin on roots, root = smallest raster index) is the same scheme.
#include "cerb_net.h"

namespace {

constexpr int TG_MAXH = CERB_TARGET_MAX_HEADS;
constexpr int TG_FAR2 = 1000000;  // 1000^2: "infinitely far" of loader/targets.py:21 as a squared distance (sqrtf gives 1000 exactly)
constexpr int TG_TILE = 16;
constexpr int TG_MAXR = 5;        // element radius of the 11 x 11 element

struct TgHeads {
    int n_heads;
    int chan[TG_MAXH];
    int ksize[TG_MAXH];
    int contour[TG_MAXH];
    int dx[TG_MAXH][2 * TG_MAXR + 1];  // row half-spans of the element: row dy (index dy + r) covers columns [-dx, +dx]
};

struct TgGeom {
    int N, H, W, C;
    int ch, cw, y0, x0;  // centre crop: rows [y0, y0 + ch), columns [x0, x0 + cw)
    int margin;          // decay margin of the weight map (10)
};

struct TgEntry {  // one inner-map label: its window [r0, r1) x [c0, c1), the offset of its distance plane, its root
    int r0, r1, c0, c1;
    long long off;
    int root, pad;
};

__device__ __forceinline__ int tg_find(const int* L, int x) {
    int p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {
        x = p;
        p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return x;
}
__device__ __forceinline__ void tg_union(int* L, int a, int b) {
    bool done;
    do {
        a = tg_find(L, a);
        b = tg_find(L, b);
        if (a < b) {
            const int old = atomicMin(&L[b], a);
            done = (old == b);
            b = old;
        } else if (b < a) {
            const int old = atomicMin(&L[a], b);
            done = (old == a);
            a = old;
        } else
            done = true;
    } while (!done);
}

// ids <- annotation channel of the head; lab <- own index / -1; flag <- 0
__global__ void tg_extract_kernel(const int32_t* __restrict__ ann, TgGeom g, TgHeads hs, int* __restrict__ ids, int* __restrict__ lab, uint8_t* __restrict__ flag) {
    const int e = blockIdx.y, hd = e / g.N, n = e % g.N;
    const int P = g.H * g.W;
    const int32_t* src = ann + (long long)n * P * g.C + hs.chan[hd];
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        const int v = src[(long long)p * g.C];
        ids[(long long)e * P + p] = v;
        lab[(long long)e * P + p] = v != 0 ? p : -1;
        flag[(long long)e * P + p] = 0;
    }
}
// lab <- own index where ids != 0, else -1 (the inner map's labelling)
__global__ void tg_init_kernel(const int* __restrict__ ids, int* __restrict__ lab, int P) {
    const long long b = (long long)blockIdx.y * P;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) lab[b + p] = ids[b + p] != 0 ? p : -1;
}
// 4-connected, predicate "equal non-zero id"
__global__ void tg_merge_kernel(const int* __restrict__ ids, int* lab, int H, int W) {
    const int P = H * W;
    const int* I = ids + (long long)blockIdx.y * P;
    int* L = lab + (long long)blockIdx.y * P;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        const int v = I[p];
        if (v == 0) continue;
        const int x = p % W;
        if (x > 0 && I[p - 1] == v) tg_union(L, p, p - 1);
        if (p >= W && I[p - W] == v) tg_union(L, p, p - W);
    }
}
// lab <- root; components with a pixel inside the centre crop are listed
__global__ void tg_flatten_listed_kernel(int* lab, uint8_t* __restrict__ flag, TgGeom g) {
    const int P = g.H * g.W;
    int* L = lab + (long long)blockIdx.y * P;
    uint8_t* F = flag + (long long)blockIdx.y * P;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        if (L[p] < 0) continue;
        const int r = tg_find(L, p);
        L[p] = r;
        const int y = p / g.W, x = p % g.W;
        if (y >= g.y0 && y < g.y0 + g.ch && x >= g.x0 && x < g.x0 + g.cw) F[r] = 1;  // every writer stores the same byte
    }
}
// lab <- root; the box of every root starts empty
__global__ void tg_flatten_box_kernel(int* lab, int4* __restrict__ box, int P) {
    int* L = lab + (long long)blockIdx.y * P;
    int4* B = box + (long long)blockIdx.y * P;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        if (L[p] < 0) continue;
        const int r = tg_find(L, p);
        L[p] = r;
        if (r == p) B[p] = make_int4(0x7fffffff, -1, 0x7fffffff, -1);
    }
}

// Inner / contour of every listed instance in one pass (loader/targets.py:84-87,131-136 summed over instances and binarised).
// The tile's labels are staged with a halo of the element's radius: 0 = background or an instance that is not listed, -1 = outside the
// image (erode and dilate both ignore such taps), root + 1 otherwise.
__global__ __launch_bounds__(TG_TILE* TG_TILE) void tg_morph_kernel(const int* __restrict__ lab, const uint8_t* __restrict__ flag, TgGeom g, TgHeads hs,
                                                                    int* __restrict__ inner_out, int32_t* __restrict__ cls_out) {
    constexpr int S = TG_TILE + 2 * TG_MAXR;
    __shared__ int tile[S * S];
    const int e = blockIdx.z, hd = e / g.N;
    const int P = g.H * g.W;
    const int* L = lab + (long long)e * P;
    const uint8_t* F = flag + (long long)e * P;
    const int r = hs.ksize[hd] >> 1;
    const int s = TG_TILE + 2 * r;
    const int by = blockIdx.y * TG_TILE, bx = blockIdx.x * TG_TILE;
    for (int i = threadIdx.x; i < s * s; i += TG_TILE * TG_TILE) {
        const int y = by - r + i / s, x = bx - r + i % s;
        int v = -1;
        if (y >= 0 && y < g.H && x >= 0 && x < g.W) {
            const int l = L[y * g.W + x];
            v = (l >= 0 && F[l]) ? l + 1 : 0;
        }
        tile[i] = v;
    }
    __syncthreads();
    const int ty = threadIdx.x / TG_TILE, tx = threadIdx.x % TG_TILE;
    const int y = by + ty, x = bx + tx;
    if (y >= g.H || x >= g.W) return;
    const int c = tile[(ty + r) * s + tx + r];
    bool all_same = c > 0, any = false;
    for (int dy = -r; dy <= r; ++dy) {
        const int dx = hs.dx[hd][dy + r];
        const int* row = tile + (ty + r + dy) * s + tx + r;
        for (int d = -dx; d <= dx; ++d) {
            const int v = row[d];
            all_same = all_same && (v == c || v < 0);
            any = any || v > 0;
        }
    }
    const int inner = all_same ? 1 : 0;
    const int contour = (!all_same && any) ? 1 : 0;
    inner_out[(long long)e * P + y * g.W + x] = inner;
    const int cy = y - g.y0, cx = x - g.x0;
    if (cy >= 0 && cy < g.ch && cx >= 0 && cx < g.cw)
        cls_out[((long long)e * g.ch + cy) * g.cw + cx] = hs.contour[hd] ? inner + 2 * contour : inner;
}

// Bounding box of every inner-map label.  Only pixels with a background (or out-of-image) 4-neighbour on the matching side can be extreme.
__global__ void tg_box_kernel(const int* __restrict__ lab, int4* box, int H, int W) {
    const int P = H * W;
    const int* L = lab + (long long)blockIdx.y * P;
    int* B = (int*)(box + (long long)blockIdx.y * P);
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        const int r = L[p];
        if (r < 0) continue;
        const int y = p / W, x = p % W;
        if (y == 0 || L[p - W] < 0) atomicMin(B + 4 * r + 0, y);
        if (y == H - 1 || L[p + W] < 0) atomicMax(B + 4 * r + 1, y);
        if (x == 0 || L[p - 1] < 0) atomicMin(B + 4 * r + 2, x);
        if (x == W - 1 || L[p + 1] < 0) atomicMax(B + 4 * r + 3, x);
    }
}
__device__ __forceinline__ TgEntry tg_window(const int4 b, int H, int W, int margin) {
    // loader/targets.py:32-38: rmax / cmax are one past the last pixel before the margin is added; clipped to the image
    TgEntry w;
    w.r0 = max(b.x - margin, 0);
    w.r1 = min(b.y + 1 + margin, H);
    w.c0 = max(b.z - margin, 0);
    w.c1 = min(b.w + 1 + margin, W);
    return w;
}
// Per image the number of labels, over all images the summed window area (what the host sizes the distance planes with) -- and, with
// `entries`, the label list itself: slot and plane offset drawn from the same counters.
__global__ void tg_list_kernel(const int* __restrict__ lab, const int4* __restrict__ box, int H, int W, int margin, int* cnt, unsigned long long* total,
                               TgEntry* __restrict__ entries, int kcap, unsigned long long area_cap) {
    const int P = H * W;
    const int e = blockIdx.y;
    const int* L = lab + (long long)e * P;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        if (L[p] != p) continue;
        TgEntry w = tg_window(box[(long long)e * P + p], H, W, margin);
        const unsigned long long area = (unsigned long long)(w.r1 - w.r0) * (unsigned long long)(w.c1 - w.c0);
        const int k = atomicAdd(cnt + e, 1);
        const unsigned long long off = atomicAdd(total, area);
        if (entries != nullptr && k < kcap) {
            if (off + area > area_cap) w.r1 = w.r0, w.off = 0;  // cannot happen with the totals of the counting pass; an empty window is never read or written
            else w.off = (long long)off;
            w.root = p;
            w.pad = 0;
            entries[(long long)e * kcap + k] = w;
        }
    }
}

// Column pass of the distance transform of one label over its window: gcol[r][c] = rows to the label's nearest pixel in column c (0xffff: none).
__global__ __launch_bounds__(64) void tg_columns_kernel(const int* __restrict__ lab, const TgEntry* __restrict__ entries, const int* __restrict__ cnt, int kcap,
                                                        int H, int W, uint16_t* __restrict__ gcol) {
    const int e = blockIdx.y, k = blockIdx.x;
    if (k >= cnt[e]) return;
    const TgEntry w = entries[(long long)e * kcap + k];
    const int* L = lab + (long long)e * H * W;
    const int ww = w.c1 - w.c0;
    uint16_t* G = gcol + w.off;
    for (int c = threadIdx.x; c < ww; c += 64) {
        int d = 0xffff;
        for (int r = w.r0; r < w.r1; ++r) {
            if (L[r * W + w.c0 + c] == w.root) d = 0;
            else if (d != 0xffff) ++d;
            G[(long long)(r - w.r0) * ww + c] = (uint16_t)d;
        }
        d = 0xffff;
        for (int r = w.r1 - 1; r >= w.r0; --r) {
            const int up = G[(long long)(r - w.r0) * ww + c];
            if (up == 0) d = 0;
            else if (d != 0xffff) ++d;
            if (d < up) G[(long long)(r - w.r0) * ww + c] = (uint16_t)d;
        }
    }
}

__device__ __forceinline__ int tg_sq(int dx, int gv) { return gv == 0xffff ? TG_FAR2 * 2 : dx * dx + gv * gv; }

// Row pass + two-nearest reduction + weight, one thread per crop pixel (loader/targets.py:46-57 and the "+ 1" of :97).
__global__ __launch_bounds__(256) void tg_weight_kernel(const int* __restrict__ lab, const TgEntry* __restrict__ entries, const int* __restrict__ cnt, int kcap, TgGeom g,
                                                        TgHeads hs, const uint16_t* __restrict__ gcol, float* __restrict__ wmap, float* __restrict__ dsum) {
    const int e = blockIdx.y, hd = e / g.N;
    const int n_lab = min(cnt[e], kcap);
    const int cp = g.ch * g.cw;
    const int* L = lab + (long long)e * g.H * g.W;
    const TgEntry* E = entries + (long long)e * kcap;
    const float sigma = (float)hs.ksize[hd];
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < cp; q += gridDim.x * blockDim.x) {
        float wv = 1.0f, ds = 2000.0f;  // fewer than two labels: no distances are computed, the map is 1 (loader/targets.py:16-17)
        if (n_lab >= 2) {
            const int y = g.y0 + q / g.cw, x = g.x0 + q % g.cw;
            int m1 = 0x7fffffff, m2 = 0x7fffffff, outside = 0;  // the two smallest of {distance^2 inside a window, 1000^2 outside it} over labels
            for (int k = 0; k < n_lab; ++k) {
                const TgEntry w = E[k];
                if (y < w.r0 || y >= w.r1 || x < w.c0 || x >= w.c1) {
                    ++outside;
                    continue;
                }
                const int ww = w.c1 - w.c0, lc = x - w.c0;
                const uint16_t* row = gcol + w.off + (long long)(y - w.r0) * ww;
                int best = tg_sq(0, row[lc]);
                for (int dx = 1; dx * dx < best; ++dx) {
                    const bool lo = lc - dx >= 0, hi = lc + dx < ww;
                    if (!lo && !hi) break;
                    if (lo) best = min(best, tg_sq(dx, row[lc - dx]));
                    if (hi) best = min(best, tg_sq(dx, row[lc + dx]));
                }
                if (best < m1) {
                    m2 = m1;
                    m1 = best;
                } else if (best < m2)
                    m2 = best;
            }
            for (int i = 0; i < min(outside, 2); ++i) {
                if (TG_FAR2 < m1) {
                    m2 = m1;
                    m1 = TG_FAR2;
                } else if (TG_FAR2 < m2)
                    m2 = TG_FAR2;
            }
            {
#pragma clang fp contract(off)
                // float32 throughout with one rounding per operation, as numpy does it: no contraction into fused multiply-adds.  The distances
                // are float64 square roots rounded to float32 -- what scipy's distance_transform_edt stored into the reference's float32 stack
                // (the single-precision __fsqrt_rn intrinsic is the hardware approximation here, 1 ulp off on some integers).
                ds = (float)sqrt((double)m1) + (float)sqrt((double)m2);
                const float xs = ds / sigma;
                const float t = -(xs * xs) / 2.0f;
                wv = L[y * g.W + x] >= 0 ? 0.0f : 10.0f * expf(t);
                wv = wv + 1.0f;
            }
        }
        wmap[(long long)e * cp + q] = wv;
        if (dsum != nullptr) dsum[(long long)e * cp + q] = ds;
    }
}

// IP / NP (binarise) and TP / PC (pass through) with the centre crop
__global__ void tg_pixel_kernel(const int32_t* __restrict__ ann, TgGeom g, TgHeads hs, int32_t* __restrict__ out) {
    const int e = blockIdx.y, hd = e / g.N, n = e % g.N;
    const int cp = g.ch * g.cw;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < cp; q += gridDim.x * blockDim.x) {
        const int y = g.y0 + q / g.cw, x = g.x0 + q % g.cw;
        const int v = ann[(((long long)n * g.H + y) * g.W + x) * g.C + hs.chan[hd]];
        out[(long long)e * cp + q] = hs.contour[hd] ? (v > 0 ? 1 : 0) : v;
    }
}

struct TgWs {
    int *ids, *lab;
    uint8_t* flag;
    int4* box;
};
size_t tg_align(size_t v) { return (v + 255) & ~(size_t)255; }
size_t tg_ws_bytes(long long E, long long P) { return tg_align(E * P * 4) * 2 + tg_align(E * P) + tg_align(E * P * 16) + 256; }
TgWs tg_carve(void* ws, long long E, long long P) {
    char* p = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    TgWs w;
    w.ids = (int*)p, p += tg_align(E * P * 4);
    w.lab = (int*)p, p += tg_align(E * P * 4);
    w.flag = (uint8_t*)p, p += tg_align(E * P);
    w.box = (int4*)p;
    return w;
}

int tg_check(const cerb_target_heads* heads, int n, int h, int w, int c, int crop_h, int crop_w, bool eroded, TgHeads* hs, TgGeom* g) {
    if (heads == nullptr || heads->n_heads < 1 || heads->n_heads > TG_MAXH) return fail("cerb_target: 1.." + std::to_string(TG_MAXH) + " heads per call");
    if (n < 1 || h < 1 || w < 1 || c < 0) return fail("cerb_target: empty annotation");  // c == 0: a call that does not read the annotation
    if (crop_h < 1 || crop_w < 1 || crop_h > h || crop_w > w) return fail("cerb_target: the crop does not fit the annotation");
    // sides below 4096: column distances are uint16 planes, squared distances stay far inside int32
    if ((long long)h * h + (long long)w * w >= (1ll << 24)) return fail("cerb_target: annotation too large (h^2 + w^2 must stay below 2^24)");
    if ((long long)n * heads->n_heads * h * w >= (1ll << 31) / 4 || (long long)n * heads->n_heads > 65535) return fail("cerb_target: batch too large for one call");
    hs->n_heads = heads->n_heads;
    for (int i = 0; i < heads->n_heads; ++i) {
        if (c > 0 && (heads->chan[i] < 0 || heads->chan[i] >= c)) return fail("cerb_target: channel index out of range");
        hs->chan[i] = heads->chan[i];
        hs->contour[i] = heads->flag[i] ? 1 : 0;
        hs->ksize[i] = heads->ksize[i];
        if (!eroded) continue;
        const int k = heads->ksize[i], r = k / 2;
        if (k < 3 || k > 2 * TG_MAXR + 1 || !(k & 1)) return fail("cerb_target: element size must be odd, 3..11");
        // OpenCV's MORPH_ELLIPSE row spans (getStructuringElement): dx = round(c * sqrt((r^2 - dy^2) / r^2)), round half to even
        for (int dy = -r; dy <= r; ++dy) hs->dx[i][dy + r] = (int)nearbyint(r * sqrt((double)(r * r - dy * dy) * (1.0 / (r * r))));
    }
    g->N = n, g->H = h, g->W = w, g->C = c;
    g->ch = crop_h, g->cw = crop_w;
    g->y0 = (int)((h - crop_h) * 0.5), g->x0 = (int)((w - crop_w) * 0.5);  // misc/utils.py:97-98
    g->margin = 10;
    return 0;
}
inline dim3 tg_grid(long long items, int E) { return dim3((unsigned)std::min<long long>((items + 255) / 256, 1024), (unsigned)E); }

}  // namespace

extern "C" size_t cerb_target_workspace_bytes(int n_images, int h, int w) { return tg_ws_bytes(n_images, (long long)h * w); }

extern "C" int cerb_target_element(int ksize, uint8_t* out) {
    if (ksize < 1 || !(ksize & 1) || out == nullptr) return fail("cerb_target_element: odd size");
    const int r = ksize / 2;
    for (int dy = -r; dy <= r; ++dy) {
        const int dx = r ? (int)nearbyint(r * sqrt((double)(r * r - dy * dy) * (1.0 / (r * r)))) : 0;
        for (int x = -r; x <= r; ++x) out[(dy + r) * ksize + x + r] = (x >= -dx && x <= dx) ? 1 : 0;
    }
    return 0;
}

extern "C" int cerb_target_pixel_maps(const int32_t* ann, int n, int h, int w, int c, const cerb_target_heads* heads, int crop_h, int crop_w, int32_t* out,
                                      void* hip_stream) {
    TgHeads hs = {};
    TgGeom g = {};
    if (tg_check(heads, n, h, w, c, crop_h, crop_w, false, &hs, &g)) return 1;
    const int E = n * hs.n_heads;
    hipLaunchKernelGGL(tg_pixel_kernel, tg_grid((long long)crop_h * crop_w, E), dim3(256), 0, (hipStream_t)hip_stream, ann, g, hs, out);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int cerb_target_eroded_maps(const int32_t* ann, int n, int h, int w, int c, const cerb_target_heads* heads, int crop_h, int crop_w, int32_t* cls_out,
                                       int32_t* meta, void* ws, size_t ws_bytes, void* hip_stream) {
    TgHeads hs = {};
    TgGeom g = {};
    if (tg_check(heads, n, h, w, c, crop_h, crop_w, true, &hs, &g)) return 1;
    const int E = n * hs.n_heads, P = h * w;
    if (ws == nullptr || ws_bytes < tg_ws_bytes(E, P)) return fail("cerb_target_eroded_maps: workspace too small (cerb_target_workspace_bytes)");
    const TgWs W = tg_carve(ws, E, P);
    hipStream_t st = (hipStream_t)hip_stream;
    const dim3 gp = tg_grid(P, E), b(256);
    hipLaunchKernelGGL(tg_extract_kernel, gp, b, 0, st, ann, g, hs, W.ids, W.lab, W.flag);
    hipLaunchKernelGGL(tg_merge_kernel, gp, b, 0, st, W.ids, W.lab, h, w);
    hipLaunchKernelGGL(tg_flatten_listed_kernel, gp, b, 0, st, W.lab, W.flag, g);
    hipLaunchKernelGGL(tg_morph_kernel, dim3((w + TG_TILE - 1) / TG_TILE, (h + TG_TILE - 1) / TG_TILE, E), dim3(TG_TILE * TG_TILE), 0, st, W.lab, W.flag, g, hs, W.ids,
                       cls_out);
    if (meta != nullptr) {  // meta[0..1] = summed window area (one 64-bit count), meta[2 + e] = labels of image e
        HIP_OK(hipMemsetAsync(meta, 0, 8 + (size_t)E * 4, st));
        hipLaunchKernelGGL(tg_init_kernel, gp, b, 0, st, W.ids, W.lab, P);
        hipLaunchKernelGGL(tg_merge_kernel, gp, b, 0, st, W.ids, W.lab, h, w);
        hipLaunchKernelGGL(tg_flatten_box_kernel, gp, b, 0, st, W.lab, W.box, P);
        hipLaunchKernelGGL(tg_box_kernel, gp, b, 0, st, W.lab, W.box, h, w);
        hipLaunchKernelGGL(tg_list_kernel, gp, b, 0, st, W.lab, W.box, h, w, g.margin, meta + 2, (unsigned long long*)meta, (TgEntry*)nullptr, 0, 0ull);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" size_t cerb_target_window_workspace_bytes(int n_images, int max_labels, unsigned long long total_area) {
    return tg_align((size_t)n_images * (size_t)std::max(max_labels, 1) * sizeof(TgEntry)) + tg_align((size_t)total_area * 2) + tg_align((size_t)n_images * 4 + 8) + 256;
}

extern "C" int cerb_target_weight_maps(int n, int h, int w, const cerb_target_heads* heads, int crop_h, int crop_w, const void* ws, size_t ws_bytes, int max_labels,
                                       unsigned long long total_area, void* win_ws, size_t win_ws_bytes, float* wmap_out, float* dsum_out, void* hip_stream) {
    TgHeads hs = {};
    TgGeom g = {};
    if (tg_check(heads, n, h, w, 0, crop_h, crop_w, true, &hs, &g)) return 1;
    const int E = n * hs.n_heads, P = h * w;
    if (ws == nullptr || ws_bytes < tg_ws_bytes(E, P)) return fail("cerb_target_weight_maps: workspace too small (cerb_target_workspace_bytes)");
    if (max_labels < 0 || max_labels > 65535) return fail("cerb_target_weight_maps: more than 65535 labels in one map");
    if (win_ws == nullptr || win_ws_bytes < cerb_target_window_workspace_bytes(E, max_labels, total_area))
        return fail("cerb_target_weight_maps: window workspace too small (cerb_target_window_workspace_bytes)");
    const TgWs W = tg_carve((void*)ws, E, P);
    const int kcap = std::max(max_labels, 1);
    char* p = (char*)(((uintptr_t)win_ws + 255) & ~(uintptr_t)255);
    TgEntry* entries = (TgEntry*)p;
    p += tg_align((size_t)E * kcap * sizeof(TgEntry));
    uint16_t* gcol = (uint16_t*)p;
    p += tg_align((size_t)total_area * 2);
    unsigned long long* total2 = (unsigned long long*)p;
    int* cnt2 = (int*)(p + 8);
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_OK(hipMemsetAsync(total2, 0, 8 + (size_t)E * 4, st));
    // the same walk over the roots as the counting pass: every label draws its slot and the offset of its plane; the totals are the ones
    // the host sized this workspace with, so every plane lies inside it
    hipLaunchKernelGGL(tg_list_kernel, tg_grid(P, E), dim3(256), 0, st, W.lab, W.box, h, w, g.margin, cnt2, total2, entries, kcap, total_area);
    if (max_labels >= 2) hipLaunchKernelGGL(tg_columns_kernel, dim3(kcap, E), dim3(64), 0, st, W.lab, entries, cnt2, kcap, h, w, gcol);
    hipLaunchKernelGGL(tg_weight_kernel, tg_grid((long long)crop_h * crop_w, E), dim3(256), 0, st, W.lab, entries, cnt2, kcap, g, hs, gcol, wmap_out, dsum_out);
    HIP_OK(hipGetLastError());
    return 0;
}
