// Instance post-processing of the Cerberus tile path on gfx950, entirely on device.  This unit: the nuclei path (front end, flood set-up, the flood
// tiers, the exact replay, cerb_postproc_nuclei).  The scans and labellers are pp_label.hip, the gland / lumen / eroded crop scheme pp_gland.hip,
// what they share pp_common.h.  Of the three only this unit reads developer switches.
//
// Replaces reference loader/postproc.py:268-407 (PostProcInstErodedContourMap.__proc_nuclei / __proc_gland /
// __proc_lumen) and the third-party routines it calls (scipy.ndimage.label / binary_fill_holes,
// skimage.morphology.remove_small_objects, skimage.segmentation.watershed, cv2.erode / dilate /
// getStructuringElement).  Integer work, HBM/latency bound -- no MFMA here.
//
// Building blocks
//   * 4-connected component labelling: lock-free union-find (atomicMin on roots), root = smallest raster index of
//     the component, so "rank of the root among roots in raster order" reproduces scipy's label numbering.
//   * component areas: wave-aggregated atomics; removal of small objects = drop roots whose area < min_size.
//   * fill holes = background components that do not touch the (image or crop) border.
//   * marker-controlled watershed: skimage's priority flood is sequential per 4-connected MASK component (floods of
//     different mask components never interact), so one WAVEFRONT owns one component and runs the exact flood with
//     a wave-cooperative 64-ary min-heap keyed by (priority value, push age, pixel index): the 64 children of a node
//     are compared with one wave-wide argmin.  Ages are assigned in skimage's neighbour order (up, left, right,
//     down), so equal-priority plateaus are split exactly as the reference splits them.  The only freedom skimage
//     leaves to its binary heap's internal layout -- the order between SEED pixels with bit-identical priority --
//     is resolved by raster index here; the floods PROVE per component whether that order can reach the label map
//     ("uncertain age" propagation, see ws_flood_kernel) and count the components where it can in n_ambiguous.
//     When the count is not zero the map is re-flooded by ws_exact_kernel: a literal emulation of skimage's ONE
//     global binary heap (all markers pushed in raster order, strict-less sift-up / sift-down) -- slow, exact.
//   * gland / lumen: per instance crop (bounding box + conditional padding) -> elliptical dilation clipped to the
//     crop -> fill holes inside the crop -> paste with "later id wins" (atomicMax).
#include <cstdio>

#include "pp_common.h"

// the watershed's start map in one pass: out[p] = mask ? 1 + rank of the root of p in the marker labelling : 0, the rank taken from the root bitmap
// (number of roots before the pixel's root in raster order; boff: the per-1024-word block offsets pp_scan_exclusive_popc left unadded, or nullptr).
// Also the smallest / largest marker label inside every mask component (lmin / lmax at the component's root LA[p]; roots_setup_kernel has initialised
// them): one pair of atomics per RUN of equal (label, component) inside a wave, and only where a plain read does not already cover the label (the
// extremes are monotone, a stale read costs an atomic, never a miss).  Taken over all labelled pixels this equals the extremes over the SEEDS (labelled
// pixels with an unlabelled mask neighbour) in every component that has an unlabelled pixel at all: a marker none of whose pixels touches an unlabelled
// mask pixel has only itself and non-mask around it, i.e. it IS its component.  Knowing them here lets ws_seed_kernel skip the single-label components.
__global__ void nuc_marker_out_bits_kernel(const int* __restrict__ L, const u64* __restrict__ bits, const int* __restrict__ wpre, const int* __restrict__ boff,
                                           const uint8_t* __restrict__ mask, int* __restrict__ out, int n, const int* __restrict__ LA, int* lmin, int* lmax) {
    const int lane = threadIdx.x & 63;
    for (long long base = (blockIdx.x * (long long)blockDim.x + threadIdx.x) - lane; base < n; base += (long long)gridDim.x * blockDim.x) {
        const long long p = base + lane;
        int v = 0, ra = -1;
        if (p < n) {
            const int r = L[p];
            if (r >= 0 && mask[p]) {
                const int w = r >> 6;
                v = wpre[w] + (boff ? boff[w / SCAN_ITEMS] : 0) + __popcll(bits[w] & ((1ull << (r & 63)) - 1ull)) + 1;
                ra = LA[p];
            }
            out[p] = v;
        }
        const int pv = __shfl_up(v, 1), pr = __shfl_up(ra, 1);
        if (v > 0 && (lane == 0 || pv != v || pr != ra)) {
            const volatile int* vmin = lmin + ra;
            const volatile int* vmax = lmax + ra;
            if (v < *vmin) atomicMin(lmin + ra, v);
            if (v > *vmax) atomicMax(lmax + ra, v);
        }
    }
}
// Four pixels per thread (W % 4 == 0, 16-byte aligned maps).  The per-pixel passes of this file are LATENCY-bound, not bandwidth-bound: 8192 resident
// waves x one dependent chain of 3 - 4 loads (~3 us under load) per 64 pixels = 0.3 - 0.5 ms per pass over 67 Mpx, whatever the bytes.  One 16-byte load
// per map and thread instead of four dword loads quarters the chains per pixel, and the common case (background) ends after the first load.
__global__ void nuc_marker_out4_kernel(const int4* __restrict__ L4, const u64* __restrict__ bits, const int* __restrict__ wpre, const int* __restrict__ boff,
                                       const uint32_t* __restrict__ mask4, int4* __restrict__ out4, long long nq, const int4* __restrict__ LA4, int* lmin,
                                       int* lmax, const uint32_t* __restrict__ mrk4) {
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
        // a start-map pixel is a marker pixel inside the mask: both byte maps are asked before any int32 map (the markers' map holds roots only in quads
        // that have a marker pixel: ccl2_final_bits4_kernel)
        const uint32_t m = mask4[q] & (mrk4[q] * 0xffu);
        if (!m) {
            out4[q] = make_int4(0, 0, 0, 0);
            continue;
        }
        const int4 l = L4[q];
        const int4 a = LA4[q];  // (same level of the load chain as L4: only labelled pixels want it, but waiting for the labels to ask costs a round trip)
        const int r[4] = {l.x, l.y, l.z, l.w};
        int v[4];
        int pr = -1, pv = 0;
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = 0;
            if (r[i] >= 0 && ((m >> (8 * i)) & 0xffu)) {
                if (r[i] != pr) {
                    const int w = r[i] >> 6;
                    pv = wpre[w] + (boff ? boff[w / SCAN_ITEMS] : 0) + __popcll(bits[w] & ((1ull << (r[i] & 63)) - 1ull)) + 1;
                    pr = r[i];
                }
                v[i] = pv;
                any = true;
            }
        }
        out4[q] = make_int4(v[0], v[1], v[2], v[3]);
        if (!any) continue;
        const int ra[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (v[i] > 0 && (i == 0 || v[i] != v[i - 1] || ra[i] != ra[i - 1])) {
                const volatile int* vmin = lmin + ra[i];
                const volatile int* vmax = lmax + ra[i];
                if (v[i] < *vmin) atomicMin(lmin + ra[i], v[i]);
                if (v[i] > *vmax) atomicMax(lmax + ra[i], v[i]);
            }
    }
}

// =================================================================================================================
// Nuclei front end
// =================================================================================================================
__global__ void nuc_threshold_kernel(const float* __restrict__ inst, long long row_stride, int pix_stride, int H, int W,
                                     uint8_t* __restrict__ msk0, uint8_t* __restrict__ mrk0, int* __restrict__ any) {
    const long long n = (long long)H * W;
    int local = 0;
    const double invW = 1.0 / (double)W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        int y, x;
        pix_yx(p, W, invW, y, x);
        const float* s = inst + y * row_stride + (long long)x * pix_stride;
        const float inner = s[0], cnt = s[1];
        const float raw = inner + cnt;  // float32 add, as numpy (postproc.py:360)
        const uint8_t m = raw > 0.5f;
        msk0[p] = m;
        mrk0[p] = inner > 0.5f;
        local |= m;
    }
    if (__any(local) && (threadIdx.x & 63) == 0) atomicOr(any, 1);
}
// Four pixels per thread (W % 4 == 0, so a quad never straddles a row and the byte maps take one 32-bit store per thread instead of four
// single-byte ones): the r04 profile had the one-pixel kernels at 2.7 TB/s of their 10 bytes per pixel.
template <bool PACKED>
__global__ void nuc_threshold4_kernel(const float* __restrict__ inst, long long row_stride, int pix_stride, int H, int W,
                                      uint32_t* __restrict__ msk0, uint32_t* __restrict__ mrk0, int* __restrict__ any) {
    const long long nq = (long long)H * W / 4;
    const int qw = W / 4;
    int local = 0;
    const double invQ = 1.0 / (double)qw;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
        int y, xq;
        pix_yx(q, qw, invQ, y, xq);
        const float* s = inst + y * row_stride + (long long)xq * 4 * pix_stride;
        uint32_t m = 0, k = 0;
        float px[8];
        if (PACKED) {  // [H][W][2] floats, 16-byte aligned rows: the quad is two 16-byte loads
            const float4 a = reinterpret_cast<const float4*>(s)[0], b = reinterpret_cast<const float4*>(s)[1];
            px[0] = a.x; px[1] = a.y; px[2] = a.z; px[3] = a.w; px[4] = b.x; px[5] = b.y; px[6] = b.z; px[7] = b.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                px[2 * i] = s[(long long)i * pix_stride];
                px[2 * i + 1] = s[(long long)i * pix_stride + 1];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float inner = px[2 * i], cnt = px[2 * i + 1];
            const float raw = inner + cnt;  // float32 add, as numpy (postproc.py:360)
            m |= (uint32_t)(raw > 0.5f) << (8 * i);
            k |= (uint32_t)(inner > 0.5f) << (8 * i);
        }
        msk0[q] = m;
        mrk0[q] = k;
        local |= (int)m;
    }
    if (__any(local) && (threadIdx.x & 63) == 0) atomicOr(any, 1);
}
// the cross erosion on four 0/1 bytes at once: AND of the word with its row neighbours and with itself shifted one byte either way (the byte
// that shifts in comes from the neighbouring word, or is 1 at the image border: the constant border never wins the min)
__global__ void erode_cross4_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int H, int W) {
    const long long nq = (long long)H * W / 4;
    const int qw = W / 4;
    const double invQ = 1.0 / (double)qw;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
        int y, xq;
        pix_yx(q, qw, invQ, y, xq);
        const uint32_t c = src[q];
        uint32_t v = c;
        if (y > 0) v &= src[q - qw];
        if (y < H - 1) v &= src[q + qw];
        const uint32_t left = xq > 0 ? src[q - 1] >> 24 : 1u, right = xq < qw - 1 ? src[q + 1] << 24 : 0x01000000u;
        v &= (c << 8) | left;
        v &= (c >> 8) | right;
        dst[q] = v;
    }
}
// cv2.erode with the 3x3 MORPH_ELLIPSE (= cross); the constant border never wins the min
__global__ void erode_cross_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W) {
    const long long n = (long long)H * W;
    const double invW = 1.0 / (double)W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        int y, x;
        pix_yx(p, W, invW, y, x);
        uint8_t v = src[p];
        if (y > 0) v &= src[p - W];
        if (y < H - 1) v &= src[p + W];
        if (x > 0) v &= src[p - 1];
        if (x < W - 1) v &= src[p + 1];
        dst[p] = v;
    }
}

// =================================================================================================================
// Watershed
// =================================================================================================================
__device__ __forceinline__ u32 order_key(float v) {  // monotone map float -> uint32 (with -0.0 == +0.0)
    if (v == 0.0f) v = 0.0f;
    const u32 b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// "Uncertain age" flag of a queue entry (top bit of its pixel / window index): the entry's position among entries of EQUAL
// priority value is not determined by (value, age) alone -- it is a seed (all seeds enter with age 0 and skimage's heap layout
// orders equal ones), or it was pushed by an entry popped inside such a tie (its age then inherits the tie's order).
#define WS_UNC32 0x80000000u
#define WS_UNC16 0x8000u

__global__ void ws_seed_kernel(const float* __restrict__ inst, long long row_stride, int pix_stride, const uint8_t* __restrict__ mask,
                               const int* __restrict__ out, const int* __restrict__ L, const int* __restrict__ hoff, int* __restrict__ hcnt,
                               u64* __restrict__ hkey, u32* __restrict__ hidx, int H, int W, int* __restrict__ unl, const int* __restrict__ lmin,
                               const int* __restrict__ lmax) {
    // lmin / lmax are final already (nuc_marker_out_bits_kernel): components whose markers carry ONE label never reach a flood
    // (ws_fill_single_kernel paints them), so neither their seeds nor their floodable-pixel counts are wanted -- isolated nuclei issue no atomic here
    const long long n = (long long)H * W;
    const double invW = 1.0 / (double)W;
    const int lane = threadIdx.x & 63;
    // whole waves step together (no lane leaves the loop early): the count of floodable pixels is added once per RUN of equal roots inside the
    // wave -- 64 consecutive pixels of a row hold a few runs, where one atomic per pixel had every ring pixel of a nucleus hit one address
    for (long long base = (blockIdx.x * (long long)blockDim.x + threadIdx.x) - lane; base < n; base += (long long)gridDim.x * blockDim.x) {
        const long long p = base + lane;
        const bool valid = p < n;
        const int o = valid ? out[p] : 0;
        const int key = (valid && !o && mask[p]) ? L[p] : -1;  // root of a floodable pixel
        const int prev = __shfl_up(key, 1);
        const bool head = key >= 0 && (lane == 0 || prev != key);
        const unsigned long long bounds = __ballot(head || key < 0);
        if (head && lmin[key] < lmax[key]) {
            const unsigned long long after = lane == 63 ? 0ull : (bounds >> (lane + 1));
            const int run = after ? __ffsll((long long)after) : 64 - lane;
            atomicAdd(&unl[key], run);
        }
        if (!o) continue;
        int y, x;
        pix_yx(p, W, invW, y, x);
        bool active = false;
        if (y > 0 && mask[p - W] && !out[p - W]) active = true;
        if (x > 0 && mask[p - 1] && !out[p - 1]) active = true;
        if (x < W - 1 && mask[p + 1] && !out[p + 1]) active = true;
        if (y < H - 1 && mask[p + W] && !out[p + W]) active = true;
        if (!active) continue;
        const int root = L[p];
        if (lmin[root] >= lmax[root]) continue;
        const int slot = hoff[root] + atomicAdd(&hcnt[root], 1);
        const float v = -inst[y * row_stride + (long long)x * pix_stride];  // watershed(-inst_inner_raw, ...)
        hkey[slot] = ((u64)order_key(v) << 32);  // age 0
        hidx[slot] = (u32)p | WS_UNC32;          // every seed's pop position among equal-valued seeds is skimage's heap layout's choice
    }
}
// bounding box of every kept mask component, keyed by its root pixel (only outline pixels issue atomics)
struct CBox {
    int y1, y2, x1, x2;  // inclusive
};
// Only components that reach a priority flood need their box (ws_worklist_bits_kernel: seeds of at least two labels, lmin < lmax; no seed at all
// leaves lmin = 0x7f7f7f7f > lmax = 0): isolated nuclei -- the common case -- skip the outline test and the atomics.
__global__ void ws_bbox_kernel(const int* __restrict__ L, const uint8_t* __restrict__ mask, CBox* bb, int H, int W, const int* __restrict__ lmin,
                               const int* __restrict__ lmax) {
    const long long n = (long long)H * W;
    const double invW = 1.0 / (double)W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        if (!mask[p]) continue;
        int y, x;
        pix_yx(p, W, invW, y, x);
        // (outline test first: its loads are neighbours of the pixel's own; the per-root gathers are then paid by ~1 mask pixel in 6)
        if (y > 0 && y < H - 1 && x > 0 && x < W - 1 && mask[p - W] && mask[p + W] && mask[p - 1] && mask[p + 1]) continue;
        const int root = L[p];
        if (lmin[root] >= lmax[root]) continue;
        CBox* b = bb + root;
        const volatile CBox* vb = b;  // monotone extremes: skip the atomic when a plain read already covers the pixel
        if (y < vb->y1) atomicMin(&b->y1, y);
        if (y > vb->y2) atomicMax(&b->y2, y);
        if (x < vb->x1) atomicMin(&b->x1, x);
        if (x > vb->x2) atomicMax(&b->x2, x);
    }
}
// floodable = in the mask and unlabelled; a seed = labelled with a floodable 4-neighbour
__device__ __forceinline__ uint32_t floodable4(uint32_t m, const int4& o) {  // byte i = 1 when pixel i is in the mask and unlabelled
    return m & ((o.x ? 0u : 1u) | (o.y ? 0u : 0x100u) | (o.z ? 0u : 0x10000u) | (o.w ? 0u : 0x1000000u));
}
// ONE pass for the seeds, the floodable-pixel counts and the boxes (round 5): all three want the same neighbourhood of a mask pixel, and the passes are
// latency-bound -- a second kernel costs its whole chain of dependent loads again (0.34 ms for the boxes alone), a few more loads in the same level of an
// existing chain cost next to nothing.  Level 1: the mask word; level 2 (threads inside the mask, 1 in 5): start map, component roots and mask words of
// the neighbourhood; level 3: the label extremes of the roots met.  Box atomics per RUN of lanes that hold outline pixels of one component in one row (the
// run's first lane carries the row and the smallest column, its last lane the largest column).
__global__ void ws_seed_bbox4_kernel(const float* __restrict__ inst, long long row_stride, int pix_stride, const uint32_t* __restrict__ mask4,
                                     const int4* __restrict__ out4, const int4* __restrict__ L4, const int* __restrict__ hoff, int* __restrict__ hcnt,
                                     u64* __restrict__ hkey, u32* __restrict__ hidx, int H, int W, int* __restrict__ unl, const int* __restrict__ lmin,
                                     const int* __restrict__ lmax, CBox* bb) {
    const long long nq = (long long)H * W / 4;
    const int qw = W / 4;
    const double invQ = 1.0 / (double)qw;
    const uint8_t* mask = (const uint8_t*)mask4;
    const int* out = (const int*)out4;
    const int lane = threadIdx.x & 63;
    for (long long q0 = (blockIdx.x * (long long)blockDim.x + threadIdx.x) - lane; q0 < nq; q0 += (long long)gridDim.x * blockDim.x) {
        const long long q = q0 + lane;
        int key = -1, y = 0, xa = 0, xb = 0;  // this thread's outline pixels of a flooded component (box run)
        const uint32_t m = q < nq ? mask4[q] : 0u;
        if (m) {  // (a label outside the mask does not exist: the start map is mask ? marker : 0)
            int xq;
            pix_yx(q, qw, invQ, y, xq);
            const bool up = y > 0, down = y < H - 1, lft = xq > 0, rgt = xq < qw - 1;
            const int4 o = out4[q];
            const int4 l = L4[q];
            const uint32_t mu = up ? mask4[q - qw] : 0u, md = down ? mask4[q + qw] : 0u;
            const uint32_t ml = lft ? mask4[q - 1] : 0u, mr = rgt ? mask4[q + 1] : 0u;
            const int root[4] = {l.x, l.y, l.z, l.w};
            const uint32_t f = floodable4(m, o);
            const uint32_t lab = m & ~f;  // bytes are 0 / 1
            // multi[i]: pixel i belongs to a component whose markers carry more than one label (the only ones that reach a flood)
            bool multi[4];
            {
                int pr = -1;
                bool pm = false;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    multi[i] = false;
                    if (!((m >> (8 * i)) & 1u)) continue;
                    if (root[i] != pr) {
                        pr = root[i];
                        pm = lmin[pr] < lmax[pr];
                    }
                    multi[i] = pm;
                }
            }
            if (multi[0] || multi[1] || multi[2] || multi[3]) {
                // floodable pixels, counted per run of equal roots inside the thread
                int i = 0;
                while (i < 4) {
                    if (!((f >> (8 * i)) & 1u) || !multi[i]) {
                        ++i;
                        continue;
                    }
                    int j = i + 1;
                    while (j < 4 && ((f >> (8 * j)) & 1u) && root[j] == root[i]) ++j;
                    atomicAdd(&unl[root[i]], j - i);
                    i = j;
                }
                // outline = mask minus its cross erosion (the image border counts as outside)
                uint32_t v = m & mu & md;
                v &= (m << 8) | (ml >> 24);
                v &= (m >> 8) | (mr << 24);
                const uint32_t outline = m & ~v;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (!((outline >> (8 * k)) & 1u) || !multi[k]) continue;
                    const int x = xq * 4 + k;
                    if (key < 0) {
                        key = root[k];
                        xa = xb = x;
                    } else if (root[k] == key) {
                        xb = x;
                    } else {  // a second component inside one thread's four pixels: on its own
                        CBox* b = bb + root[k];
                        const volatile CBox* vb = b;
                        if (y < vb->y1) atomicMin(&b->y1, y);
                        if (y > vb->y2) atomicMax(&b->y2, y);
                        if (x < vb->x1) atomicMin(&b->x1, x);
                        if (x > vb->x2) atomicMax(&b->x2, x);
                    }
                }
                // seeds: labelled pixels with a floodable 4-neighbour
                if (lab) {
                    uint32_t nb = (f << 8) | (f >> 8);  // left / right neighbours inside the word
                    // (fetched here, one round trip later than the rest: hoisting the two 16-byte loads to every mask thread measured 0.07 ms slower)
                    if (mu) nb |= floodable4(mu, out4[q - qw]);
                    if (md) nb |= floodable4(md, out4[q + qw]);
                    const long long p0 = q * 4;
                    if ((lab & 1u) && (ml >> 24) && !out[p0 - 1]) nb |= 1u;
                    if ((lab & 0x1000000u) && (mr & 0xffu) && !out[p0 + 4]) nb |= 0x1000000u;
                    const uint32_t act = lab & nb;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (!((act >> (8 * k)) & 1u) || !multi[k]) continue;
                        const int r = root[k];
                        const int slot = hoff[r] + atomicAdd(&hcnt[r], 1);
                        const float val = -inst[y * row_stride + (long long)(xq * 4 + k) * pix_stride];  // watershed(-inst_inner_raw, ...)
                        hkey[slot] = ((u64)order_key(val) << 32);  // age 0
                        hidx[slot] = (u32)(p0 + k) | WS_UNC32;     // every seed's pop position among equal-valued seeds is skimage's heap layout's choice
                    }
                }
            }
        }
        const int pk = __shfl_up(key, 1), py = __shfl_up(y, 1), nk = __shfl_down(key, 1), ny = __shfl_down(y, 1);
        if (key >= 0) {
            CBox* b = bb + key;
            const volatile CBox* vb = b;
            if (lane == 0 || pk != key || py != y) {
                if (y < vb->y1) atomicMin(&b->y1, y);
                if (y > vb->y2) atomicMax(&b->y2, y);
                if (xa < vb->x1) atomicMin(&b->x1, xa);
            }
            if (lane == 63 || nk != key || ny != y)
                if (xb > vb->x2) atomicMax(&b->x2, xb);
        }
    }
    (void)mask;
}
// Compact lists of component roots that own at least one seed, in three tiers:
//   window tier : bounding box (+1 px ring) fits WS_WIN_CAP pixels and area <= WS_LDS_CAP -> whole flood in LDS   (front of wl)
//   LDS-heap tier: area <= WS_LDS_CAP                                                     -> heap in LDS           (wl2)
//   global tier : everything else                                                        -> heap in global memory (back of wl)
//   big-window  : bounding box fits WS_BIGWIN_CAP pixels and (seeds + unlabelled mask pixels) <= WS_BIGHEAP_CAP: one wave per
//                 workgroup with ~150 KB of LDS                                                                  (wl3)
#define WS_LDS_CAP 1024
#define WS_WIN_CAP 2304
#define WS_TINY_CAP 512    // tiny-window tier: pairs / small clusters; 13 KB of LDS per wave -> 12 waves per CU instead of 4
#define WS_TINY_WIN 1024
#define WS_BIGWIN_CAP 16384
#define WS_BIGHEAP_CAP 2048
// A component all of whose seeds carry ONE label needs no priority flood: every unlabelled mask pixel of a 4-connected mask
// component is reachable from a seed through unlabelled mask pixels, so the flood can only ever assign that label
// (ws_fill_single_kernel).  Isolated nuclei -- the common case -- take this path; only touching clusters reach the heaps.

// Per-component setup over the root bitmap (one thread per 64-pixel word): counters, label extremes, box, and the heap offset -- any disjoint
// partition of the heap arrays will do (the floods address their heap as hoff[root] + i), so a block adds the areas of its roots up and takes its
// range with ONE atomic; no exclusive scan over the pixel map is needed.  The per-root arrays are indexed by root pixel and only ever read at kept roots, so
// initialising them HERE replaces four whole-map fills.
__global__ __launch_bounds__(256) void roots_setup_kernel(const u64* __restrict__ bits, int nw, const int* __restrict__ area, int* __restrict__ hoff,
                                                          int* __restrict__ hcnt, int* __restrict__ unl, int* __restrict__ lmin, int* __restrict__ lmax,
                                                          CBox* __restrict__ bb, int H, int W, int* __restrict__ total) {
    __shared__ int bbase;
    const int tid = threadIdx.x;
    const int w = blockIdx.x * 256 + tid;
    const u64 word = w < nw ? bits[w] : 0ull;
    int tsum = 0;
    for (u64 b = word; b; b &= b - 1) tsum += area[(long long)w * 64 + (__ffsll((long long)b) - 1)];
    int tot;
    int run = block_exclusive_scan_256(tsum, tot);
    if (tid == 255) bbase = tot ? atomicAdd(total, tot) : 0;  // (the last thread holds the block's sum)
    __syncthreads();
    run += bbase;
    for (u64 b = word; b; b &= b - 1) {
        const long long j = (long long)w * 64 + (__ffsll((long long)b) - 1);
        hoff[j] = run;
        run += area[j];
        hcnt[j] = 0;
        unl[j] = 0;
        lmin[j] = 0x7f7f7f7f;
        lmax[j] = 0;
        bb[j] = CBox{H, -1, W, -1};
    }
}
__global__ void ws_worklist_bits_kernel(const u64* __restrict__ bits, int nw, const int* __restrict__ hcnt, const int* __restrict__ area,
                                        const int* __restrict__ unl, const CBox* __restrict__ bb, const int* __restrict__ lmin, const int* __restrict__ lmax,
                                        int* __restrict__ wl, int* __restrict__ wl2, int* __restrict__ wl3, int* __restrict__ wl4, int* __restrict__ counts, int n) {
    for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += gridDim.x * blockDim.x)
        for (u64 bw = bits[w]; bw; bw &= bw - 1) {
            const int p = w * 64 + (__ffsll((long long)bw) - 1);
            if (!(hcnt[p] > 0 && lmin[p] != lmax[p])) continue;
            const CBox b = bb[p];
            const long long win = (long long)(b.y2 - b.y1 + 3) * (b.x2 - b.x1 + 3);
            const int need = hcnt[p] + unl[p];  // every queue entry is a seed or a pixel that was unlabelled at the start
            if (need <= WS_TINY_CAP && win <= WS_TINY_WIN) wl4[atomicAdd(counts + 4, 1)] = p;
            else if (need <= WS_LDS_CAP && win <= WS_WIN_CAP) wl[atomicAdd(counts + 0, 1)] = p;
            else if (need <= WS_BIGHEAP_CAP && win <= WS_BIGWIN_CAP) wl3[atomicAdd(counts + 3, 1)] = p;
            else if (area[p] <= WS_LDS_CAP) wl2[atomicAdd(counts + 1, 1)] = p;
            else wl[n - 1 - atomicAdd(counts + 2, 1)] = p;
        }
}

__global__ void ws_fill_single_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ L, const int* __restrict__ lmin,
                                      const int* __restrict__ lmax, int* __restrict__ out, int n) {
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        if (!mask[p] || out[p]) continue;
        const int r = L[p];
        const int a = lmin[r];
        if (a == lmax[r]) out[p] = a;
    }
}

// four pixels per thread (W % 4 == 0, 16-byte aligned maps): one word of the mask decides whether the quad's labels are looked at at all
__global__ void ws_fill_single4_kernel(const uint32_t* __restrict__ mask4, const int4* __restrict__ L4, const int* __restrict__ lmin, const int* __restrict__ lmax,
                                       int4* __restrict__ out4, long long nq) {
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
        const uint32_t mw = mask4[q];
        if (!mw) continue;
        int4 o = out4[q];
        int v[4] = {o.x, o.y, o.z, o.w};
        bool need = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) need = need || (((mw >> (8 * i)) & 0xffu) && !v[i]);
        if (!need) continue;
        const int4 l = L4[q];
        const int r[4] = {l.x, l.y, l.z, l.w};
        int pr = -1, pa = 0;
        bool single = false;
        int* out = reinterpret_cast<int*>(out4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!((mw >> (8 * i)) & 0xffu) || v[i]) continue;
            if (r[i] != pr) {
                pr = r[i];
                pa = lmin[pr];
                single = pa == lmax[pr];
            }
            // one store per pixel, never the whole quad: the flood tiers run beside this kernel on other streams and may be writing the quad's other pixels
            if (single) out[q * 4 + i] = pa;
        }
    }
}

__device__ __forceinline__ bool hless(u64 k1, u32 i1, u64 k2, u32 i2) { return k1 < k2 || (k1 == k2 && i1 < i2); }

// wave-wide min of a u32: 4 DPP row rotations (min inside each 16-lane row), then the 4 row results via readlane.
__device__ __forceinline__ u32 wave_min_u32(u32 v) {
    v = min(v, (u32)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x121, 0xf, 0xf, false));  // row_ror:1
    v = min(v, (u32)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x122, 0xf, 0xf, false));  // row_ror:2
    v = min(v, (u32)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x124, 0xf, 0xf, false));  // row_ror:4
    v = min(v, (u32)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x128, 0xf, 0xf, false));  // row_ror:8
    const u32 r0 = (u32)__builtin_amdgcn_readlane((int)v, 0), r1 = (u32)__builtin_amdgcn_readlane((int)v, 16);
    const u32 r2 = (u32)__builtin_amdgcn_readlane((int)v, 32), r3 = (u32)__builtin_amdgcn_readlane((int)v, 48);
    return min(min(r0, r1), min(r2, r3));
}
// wave-wide argmin of (key, idx), lexicographic (priority value, age, pixel index); every lane returns the winning lane id
__device__ __forceinline__ int wave_argmin(u64 k, u32 i, bool valid, u64* kout, u32* iout) {
    const u32 hi = valid ? (u32)(k >> 32) : ~0u;
    const u32 mh = wave_min_u32(hi);
    const bool c1 = valid && hi == mh;
    const u32 ml = wave_min_u32(c1 ? (u32)k : ~0u);
    const bool c2 = c1 && (u32)k == ml;
    const u32 mi = wave_min_u32(c2 ? i : ~0u);
    const u64 win = __ballot(c2 && i == mi);
    *kout = ((u64)mh << 32) | ml;
    *iout = mi;
    return win ? __ffsll((long long)win) - 1 : 0;
}

// 64-ary heap, node i has children 64 i + 1 .. 64 i + 64.  All lanes call these with uniform arguments.
// PAYLOAD: entries carry a value of hl beside (key, index) that moves with them and has no part in the order (pl: the payload of the entry placed).
// POS: type of the child positions -- 64 i + 1 is computed before it is compared with n, and passes 2^31 in a heap of more than 2^25 entries.
template <bool PAYLOAD = false, typename POS = long long>
__device__ __forceinline__ void heap_sift_down(volatile u64* hk, volatile u32* hi, int n, int i, u64 k, u32 x, volatile int* hl = nullptr, int pl = 0) {
    const int lane = threadIdx.x & 63;
    for (;;) {
        const POS c0 = (POS)64 * i + 1;
        if (c0 >= n) break;
        const POS c = c0 + lane;
        const bool valid = c < n;
        const u64 ck = valid ? hk[c] : 0;
        const u32 ci = valid ? hi[c] : 0;
        u64 mk;
        u32 mi;
        const int ml = wave_argmin(ck, ci, valid, &mk, &mi);
        if (!hless(mk, mi, k, x)) break;
        int ml_pl = 0;
        if (PAYLOAD) ml_pl = hl[c0 + ml];
        if (lane == 0) {
            hk[i] = mk;
            hi[i] = mi;
            if (PAYLOAD) hl[i] = ml_pl;
        }
        i = (int)(c0 + ml);
    }
    if (lane == 0) {
        hk[i] = k;
        hi[i] = x;
        if (PAYLOAD) hl[i] = pl;
    }
}
template <bool PAYLOAD = false>
__device__ __forceinline__ void heap_push(volatile u64* hk, volatile u32* hi, int* n, u64 k, u32 x, volatile int* hl = nullptr, int pl = 0) {
    int j = (*n)++;
    while (j > 0) {
        const int par = (j - 1) >> 6;
        const u64 pk = hk[par];
        const u32 pi = hi[par];
        if (!hless(k, x, pk, pi)) break;
        int par_pl = 0;
        if (PAYLOAD) par_pl = hl[par];
        if ((threadIdx.x & 63) == 0) {
            hk[j] = pk;
            hi[j] = pi;
            if (PAYLOAD) hl[j] = par_pl;
        }
        j = par;
    }
    if ((threadIdx.x & 63) == 0) {
        hk[j] = k;
        hi[j] = x;
        if (PAYLOAD) hl[j] = pl;
    }
}

// One wavefront per mask component.  Exact sequential priority flood (skimage _watershed_cy.watershed_raveled,
// compactness 0, no watershed line): pop min (value, age); for neighbours in order up, left, right, down: if in mask
// and unlabelled -> label it NOW with the popped pixel's label, age += 1, push.
//
// Tie rule (all flood kernels; validated on the CPU against the oracle's literal heap by tests/tools/dev_tie_rule_fuzz.py).
// (value, age) is a total order except between age-0 seeds of equal value, where skimage's global heap layout decides and this
// kernel takes raster order instead.  That choice reaches the label map only through
//   (a) a DIRECT conflict: the popped entry X labels a pixel q that also touches an equal-valued pixel of ANOTHER label
//       (whichever of the two pops first claims q), or
//   (b) the AGES of the pixels X pushes, which inherit X's position inside its tie and matter again only where such
//       children tie in value among themselves -- so pushed entries carry the "uncertain age" flag of WS_UNC32 and rule (a) is
//       applied to them in turn, and
//   (c) a child that is smaller than the tied value itself: it pops before the rest of the tie, which the bookkeeping of
//       (b) assumes cannot happen (conservatively counted as ambiguous).
// X is "inside a tie" when it carries the flag and the entry popped before it or the one popped after it has X's value.
// A component where none of (a)/(c) fires is labelled identically under every tie order, skimage's included.
__device__ __forceinline__ bool ws_conflict_global(const float* __restrict__ inst, long long row_stride, int pix_stride, const int* out, long long q,
                                                   long long p, int lab, u32 v, int H, int W) {
    const int qy = (int)(q / W), qx = (int)(q % W);
    bool hit = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int wy = qy + (j == 0 ? -1 : j == 3 ? 1 : 0), wx = qx + (j == 1 ? -1 : j == 2 ? 1 : 0);
        if (wy < 0 || wy >= H || wx < 0 || wx >= W) continue;
        const long long w = (long long)wy * W + wx;
        if (w == p) continue;
        const int ow = __hip_atomic_load(&out[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ow != 0 && ow != lab && order_key(-inst[wy * row_stride + (long long)wx * pix_stride]) == v) hit = true;
    }
    return hit;
}

// Work items are handed out one at a time (a counter per tier, zeroed with the call's scratch words): the floods of a tier differ several-fold in
// length, and a static stride over the list left a tier waiting for the wave that happened to draw the long ones.
__device__ __forceinline__ int ws_next_item(int* next) {
    int v = 0;
    if ((threadIdx.x & 63) == 0) v = atomicAdd(next, 1);
    return __shfl(v, 0);
}
__global__ __launch_bounds__(256) void ws_flood_kernel(const float* __restrict__ inst, long long row_stride, int pix_stride,
                                                       const uint8_t* __restrict__ mask, int* out, const int* __restrict__ wl,
                                                       const int* __restrict__ wl_n, const int* __restrict__ hoff, const int* __restrict__ hcnt,
                                                       u64* hkey, u32* hidx, int H, int W, int* __restrict__ n_ambiguous, int wl_len, int* next) {
    const int lane = threadIdx.x & 63;
    for (int w = ws_next_item(next); w < *wl_n; w = ws_next_item(next)) {
        const int root = wl[wl_len - 1 - w];  // large-component list grows from the back of wl
        volatile u64* hk = hkey + hoff[root];
        volatile u32* hi = hidx + hoff[root];
        int n = hcnt[root];
        // heapify (Floyd): sift down every internal node, last to first
        for (int i = (n - 2) >> 6; i >= 0 && n > 1; --i) {
            const u64 k = hk[i];
            const u32 x = hi[i];
            heap_sift_down(hk, hi, n, i, k, x);
        }
        u32 age = 0;
        bool have_prev = false, ambiguous = false;
        u32 prev_val = 0;
        while (n > 0) {
            const u64 k = hk[0];
            const u32 pu = hi[0];
            const u32 p = pu & ~WS_UNC32;
            --n;
            if (n > 0) {
                const u64 lk = hk[n];
                const u32 li = hi[n];
                heap_sift_down(hk, hi, n, 0, lk, li);
            }
            const int lab = __hip_atomic_load(&out[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const u32 v = (u32)(k >> 32);
            bool tied = have_prev && prev_val == v;
            if (!tied && n > 0) tied = (u32)(hk[0] >> 32) == v;  // the new minimum
            const bool unc = (pu & WS_UNC32) && tied;
            have_prev = true;
            prev_val = v;
            const int y = (int)(p / (u32)W), x = (int)(p % (u32)W);
            // lanes 0..3 look at the four neighbours in skimage's order: up, left, right, down
            long long q = -1;
            if (lane == 0 && y > 0) q = (long long)p - W;
            if (lane == 1 && x > 0) q = (long long)p - 1;
            if (lane == 2 && x < W - 1) q = (long long)p + 1;
            if (lane == 3 && y < H - 1) q = (long long)p + W;
            bool elig = false;
            u32 vq = 0;
            if (q >= 0 && mask[q]) {
                elig = __hip_atomic_load(&out[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
                if (elig) {
                    __hip_atomic_store(&out[q], lab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const int qy = (int)(q / W), qx = (int)(q % W);
                    vq = order_key(-inst[qy * row_stride + (long long)qx * pix_stride]);
                }
            }
            if (unc && elig && (vq < v || ws_conflict_global(inst, row_stride, pix_stride, out, q, p, lab, v, H, W))) ambiguous = true;
            const u64 em = __ballot(elig);
            for (int t = 0; t < 4; ++t) {
                if (!((em >> t) & 1)) continue;
                ++age;
                const u32 qk = (u32)__shfl((int)vq, t);
                const u32 qi = (u32)__shfl((int)q, t) | (unc ? WS_UNC32 : 0u);
                heap_push(hk, hi, &n, ((u64)qk << 32) | age, qi);
            }
        }
        if (__any(ambiguous) && lane == 0) atomicAdd(n_ambiguous, 1);
    }
}

// Window tier: the whole flood of a small component runs out of LDS.  Per wave: a (bbox + 1 px ring) window with the
// per-pixel state (-1 outside this component's mask, 0 unlabelled, > 0 label) and the monotone-mapped priority, plus the
// 64-ary heap (key = priority << 32 | age, index = window index, whose order equals raster order inside the component).
// Seeds are found by the wave itself; no global memory is touched between the window load and the final write-back.
template <int WIN_CAP, int HEAP_CAP, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void ws_flood_window_kernel(const float* __restrict__ inst, long long row_stride, int pix_stride,
                                                                     const uint8_t* __restrict__ mask, const int* __restrict__ L, int* out,
                                                                     const int* __restrict__ wl, const int* __restrict__ wl_n,
                                                                     const CBox* __restrict__ bb, int H, int W, int* __restrict__ n_ambiguous, int* next) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    constexpr size_t PER_WAVE = (size_t)HEAP_CAP * 8 + (size_t)WIN_CAP * 8 + (size_t)HEAP_CAP * 2;
    unsigned char* mine = s_raw + (size_t)wv * PER_WAVE;
    volatile u64* hk = reinterpret_cast<u64*>(mine);
    volatile int* st = reinterpret_cast<int*>(mine + (size_t)HEAP_CAP * 8);
    volatile u32* vl = reinterpret_cast<u32*>(mine + (size_t)HEAP_CAP * 8 + (size_t)WIN_CAP * 4);
    volatile unsigned short* hi = reinterpret_cast<unsigned short*>(mine + (size_t)HEAP_CAP * 8 + (size_t)WIN_CAP * 8);
    for (int w = ws_next_item(next); w < *wl_n; w = ws_next_item(next)) {
        const int root = wl[w];
        const CBox b = bb[root];
        const int wh = b.y2 - b.y1 + 3, ww = b.x2 - b.x1 + 3, wn = wh * ww;
        // ---- load the window -----------------------------------------------------------------------------------------
        for (int i = lane; i < wn; i += 64) {
            const int y = b.y1 - 1 + i / ww, x = b.x1 - 1 + i % ww;
            int s = -1;
            u32 v = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const long long p = (long long)y * W + x;
                if (mask[p] && L[p] == root) {
                    s = out[p];
                    v = order_key(-inst[y * row_stride + (long long)x * pix_stride]);
                }
            }
            st[i] = s;
            vl[i] = v;
        }
        // ---- seeds: labelled pixels with an unlabelled in-mask neighbour (window order == raster order) -----------------
        int n = 0;
        for (int i0 = 0; i0 < wn; i0 += 64) {
            const int i = i0 + lane;
            bool seed = false;
            if (i < wn && st[i] > 0) seed = st[i - ww] == 0 || st[i - 1] == 0 || st[i + 1] == 0 || st[i + ww] == 0;
            const u64 m = __ballot(seed);
            if (seed) {
                const int slot = n + __popcll(m & ((1ull << lane) - 1));
                hk[slot] = (u64)vl[i] << 32;  // age 0
                hi[slot] = (unsigned short)(i | WS_UNC16);
            }
            n += __popcll(m);
        }
        // ---- flood with an UNORDERED queue: the frontier of a nucleus cluster is a few dozen to a few hundred entries, so the
        // minimum is found by one strided scan (each lane keeps the best of its entries) + one wave-wide argmin, the popped slot is
        // refilled with the last entry and the (up to four) pushes are plain appends done by lanes 0..3 in parallel.  Same total
        // order as the heap ((value, age), then window index), hence the same pops.  Tie rule: see ws_flood_kernel.
        u32 age = 0;
        bool have_prev = false, ambiguous = false;
        u32 prev_val = 0;
        while (n > 0) {
            u64 bk = ~0ull;
            u32 bi = ~0u;
            int bpos = -1, bc = 0;  // bc: how many of this lane's entries carry the lane's smallest VALUE
            {
                // four strided entries per lane and trip: the LDS reads of a trip are independent, so their latencies overlap
                // (plain pointers for that; the empty asm keeps the compiler from carrying queue contents across pops)
                asm volatile("" ::: "memory");
                const u64* hkq = const_cast<const u64*>(hk);
                const unsigned short* hiq = const_cast<const unsigned short*>(hi);
                for (int c = lane; c < n; c += 256) {
                    u64 ck[4];
                    u32 ci[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int cc = c + 64 * u;
                        const bool in = cc < n;
                        ck[u] = in ? hkq[cc] : ~0ull;
                        ci[u] = in ? (u32)hiq[cc] : ~0u;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (c + 64 * u < n) {
                            const u32 cv = (u32)(ck[u] >> 32), bv = (u32)(bk >> 32);
                            bc = (bpos < 0 || cv < bv) ? 1 : bc + (cv == bv);
                            if (bpos < 0 || hless(ck[u], ci[u], bk, bi)) {
                                bk = ck[u];
                                bi = ci[u];
                                bpos = c + 64 * u;
                            }
                        }
                }
                asm volatile("" ::: "memory");
            }
            u64 k;
            u32 wi_u;
            const int wl_ = wave_argmin(bk, bi, bpos >= 0, &k, &wi_u);
            const int pos = __shfl(bpos, wl_);
            const int wi = (int)(wi_u & ~WS_UNC16);
            const int lab = st[wi];
            const u32 v = (u32)(k >> 32);
            // another queue entry with the popped value?  (two lanes hold one, or one lane holds two)
            const bool mine = bpos >= 0 && (u32)(bk >> 32) == v;
            const u64 holders = __ballot(mine);
            const bool tied = (have_prev && prev_val == v) || __popcll(holders) >= 2 || __ballot(mine && bc >= 2) != 0;
            const bool unc = (wi_u & WS_UNC16) && tied;
            have_prev = true;
            prev_val = v;
            --n;
            if (lane == 0 && pos != n) {
                hk[pos] = hk[n];
                hi[pos] = hi[n];
            }
            // lanes 0..3: up, left, right, down (skimage's neighbour order); the ring of -1 makes bounds checks unnecessary
            const int nq = wi + (lane == 0 ? -ww : lane == 1 ? -1 : lane == 2 ? 1 : ww);
            bool elig = false;
            if (lane < 4) elig = st[nq] == 0;
            const u64 em = __ballot(elig);
            if (elig) {
                const int before = __popcll(em & ((1ull << lane) - 1));
                const u32 vq = vl[nq];
                st[nq] = lab;
                hk[n + before] = ((u64)vq << 32) | (u64)(age + 1 + before);
                hi[n + before] = (unsigned short)(nq | (unc ? WS_UNC16 : 0u));
                if (unc) {
                    if (vq < v) ambiguous = true;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int wq = nq + (j == 0 ? -ww : j == 1 ? -1 : j == 2 ? 1 : ww);
                        if (wq == wi) continue;
                        const int sw = st[wq];
                        if (sw > 0 && sw != lab && vl[wq] == v) ambiguous = true;
                    }
                }
            }
            const int np = __popcll(em);
            n += np;
            age += np;
        }
        // ---- write back -----------------------------------------------------------------------------------------------------
        for (int i = lane; i < wn; i += 64) {
            const int s = st[i];
            if (s > 0) out[(long long)(b.y1 - 1 + i / ww) * W + (b.x1 - 1 + i % ww)] = s;
        }
        if (__any(ambiguous) && lane == 0) atomicAdd(n_ambiguous, 1);
    }
}

// Same flood, heap in LDS (one 1024-entry heap per wave; the heap never exceeds the component's area) with the label kept
// beside the pixel index, and the neighbour probe fused into ONE global round trip per pop (mask, label and priority of the
// four neighbours are fetched together by lanes 0..3).
__global__ __launch_bounds__(256) void ws_flood_lds_kernel(const float* __restrict__ inst, long long row_stride, int pix_stride,
                                                           const uint8_t* __restrict__ mask, int* out, const int* __restrict__ wl,
                                                           const int* __restrict__ wl_n, const int* __restrict__ hoff,
                                                           const int* __restrict__ hcnt, const u64* __restrict__ hkey,
                                                           const u32* __restrict__ hidx, int H, int W, int* __restrict__ n_ambiguous, int* next) {
    __shared__ u64 s_key[4][WS_LDS_CAP];
    __shared__ u32 s_idx[4][WS_LDS_CAP];
    __shared__ int s_lab[4][WS_LDS_CAP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    volatile u64* hk = s_key[wv];
    volatile u32* hi = s_idx[wv];
    volatile int* hl = s_lab[wv];
    for (int w = ws_next_item(next); w < *wl_n; w = ws_next_item(next)) {
        const int root = wl[w];
        int n = hcnt[root];
        const int base = hoff[root];
        for (int i = lane; i < n; i += 64) {
            const u32 px = hidx[base + i];
            hk[i] = hkey[base + i];
            hi[i] = px;
            hl[i] = out[px & ~WS_UNC32];
        }
        // heapify (Floyd) -- (key, idx) order; the label rides along
        for (int i = (n - 2) >> 6; i >= 0 && n > 1; --i) {
            const u64 k = hk[i];
            const u32 x = hi[i];
            const int lb = hl[i];
            heap_sift_down<true, int>(hk, hi, n, i, k, x, hl, lb);
        }
        u32 age = 0;
        bool have_prev = false, ambiguous = false;
        u32 prev_val = 0;
        while (n > 0) {
            const u64 k = hk[0];
            const u32 pu = hi[0];
            const u32 p = pu & ~WS_UNC32;
            const int lab = hl[0];
            --n;
            if (n > 0) {  // move the last entry to the root and sift it down
                const u64 lk = hk[n];
                const u32 li = hi[n];
                const int ll = hl[n];
                heap_sift_down<true, int>(hk, hi, n, 0, lk, li, hl, ll);
            }
            // tie rule: see ws_flood_kernel
            const u32 v = (u32)(k >> 32);
            bool tied = have_prev && prev_val == v;
            if (!tied && n > 0) tied = (u32)(hk[0] >> 32) == v;
            const bool unc = (pu & WS_UNC32) && tied;
            have_prev = true;
            prev_val = v;
            const int y = (int)(p / (u32)W), x = (int)(p % (u32)W);
            long long q = -1;
            if (lane == 0 && y > 0) q = (long long)p - W;
            if (lane == 1 && x > 0) q = (long long)p - 1;
            if (lane == 2 && x < W - 1) q = (long long)p + 1;
            if (lane == 3 && y < H - 1) q = (long long)p + W;
            bool elig = false;
            u32 vq = 0;
            if (q >= 0) {
                // one round trip: mask, current label and priority of the neighbour
                const uint8_t mq = mask[q];
                const int oq = __hip_atomic_load(&out[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int qy = (int)(q / W), qx = (int)(q % W);
                vq = order_key(-inst[qy * row_stride + (long long)qx * pix_stride]);
                elig = mq && oq == 0;
                if (elig) __hip_atomic_store(&out[q], lab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (unc && elig && (vq < v || ws_conflict_global(inst, row_stride, pix_stride, out, q, p, lab, v, H, W))) ambiguous = true;
            const u64 em = __ballot(elig);
            for (int t = 0; t < 4; ++t) {
                if (!((em >> t) & 1)) continue;
                ++age;
                const u64 nk = ((u64)(u32)__shfl((int)vq, t) << 32) | age;
                const u32 nx = (u32)__shfl((int)q, t) | (unc ? WS_UNC32 : 0u);
                heap_push<true>(hk, hi, &n, nk, nx, hl, lab);
            }
        }
        if (__any(ambiguous) && lane == 0) atomicAdd(n_ambiguous, 1);
    }
}

// =================================================================================================================
// Exact tie order: literal emulation of skimage's global heap (runs only when a flood flagged an ambiguous component)
// =================================================================================================================
// skimage.segmentation.watershed keeps ONE binary heap for the whole image (_watershed_cy.pyx + _shared/heap_general.pxi;
// the checker's C restatement of it is pinned against the real library): every marker pixel is pushed in
// raster order with age 0, `smaller` is strict on (value, age), heappush sifts up while the new entry is smaller than its
// parent, heappop moves the LAST entry to the root and sifts it down preferring the left child on equal keys.  The order in
// which equal-valued markers leave that heap is a function of its whole push / pop history, so it cannot be evaluated per
// component: one wavefront replays the history.  The replay is literal (same array layout, same comparisons) but each heap
// operation is wave-cooperative: a pop gathers the six levels below the hole with one load per lane pair (126 descendants),
// walks them in registers (readlane) and repeats; a push gathers all <= 31 ancestors of the new leaf at once, and -- the path
// being sorted -- shifts the ancestors that are larger down by one in a single scatter.  Heap positions [0, 8191) (13 levels)
// live in LDS, deeper ones in global memory; the four neighbour probes of a pop are issued before its sift-down.
#define EX_LDS 8191
struct ExHeap {
    volatile u64* sk;
    volatile u32* si;
    u64* gk;
    u32* gi;
};
// Only this one wave ever touches the heap, so no agent-scope coherence is needed: workgroup-scope accesses stay in the CU's own
// L1 / the XCD's L2 (an agent-scope load has to miss both L2-non-coherent levels on a multi-XCD part: ~2 us per dependent access).
__device__ __forceinline__ void ex_load(const ExHeap& h, long long pos, u64& k, u32& i) {
    if (pos < EX_LDS) {
        k = h.sk[pos];
        i = h.si[pos];
    } else {
        k = __hip_atomic_load(&h.gk[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        i = __hip_atomic_load(&h.gi[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}
__device__ __forceinline__ void ex_store(const ExHeap& h, long long pos, u64 k, u32 i) {
    if (pos < EX_LDS) {
        h.sk[pos] = k;
        h.si[pos] = i;
    } else {
        __hip_atomic_store(&h.gk[pos], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_store(&h.gi[pos], i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}
__device__ __forceinline__ u32 ex_uni(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ u64 ex_uni64(u64 v) { return ((u64)ex_uni((u32)(v >> 32)) << 32) | ex_uni((u32)v); }
__device__ __forceinline__ u64 ex_lane64(u64 v, int l) {
    return ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), l) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)v, l);
}
// position of local node j (0 = the hole, children 2j+1 / 2j+2) of the subtree rooted at heap position i
__device__ __forceinline__ long long ex_pos(long long i, int j) {
    const int d = 31 - __clz(j + 1);
    return ((i + 1) << d) - 1 + (j + 1 - (1 << d));
}
// heappop's tail: entry x (the former last entry) enters at the root of a heap of n entries and sifts down
__device__ __forceinline__ void ex_sift_down(const ExHeap& h, int n, u64 xk, u32 xi) {
    const int lane = threadIdx.x & 63;
    long long i = 0;
    for (;;) {
        u64 ka = 0, kb = 0;
        u32 ia = 0, ib = 0;
        if (lane >= 1) {
            const long long pa = ex_pos(i, lane);
            if (pa < n) ex_load(h, pa, ka, ia);
        }
        if (lane <= 62) {
            const long long pb = ex_pos(i, lane + 64);
            if (pb < n) ex_load(h, pb, kb, ib);
        }
        int cur = 0;
        bool placed = false;
#pragma unroll 1
        for (int step = 0; step < 6; ++step) {
            const int l = 2 * cur + 1, r = l + 1;
            const long long pl = ex_pos(i, l);
            if (pl >= n) {
                placed = true;
                break;
            }
            const u64 kl = l < 64 ? ex_lane64(ka, l) : ex_lane64(kb, l - 64);
            int s = cur;
            u64 ks = xk;
            if (kl < xk) {  // smaller(l, i)
                s = l;
                ks = kl;
            }
            if (pl + 1 < n) {
                const u64 kr = r < 64 ? ex_lane64(ka, r) : ex_lane64(kb, r - 64);
                if (kr < ks) s = r;  // smaller(r, smallest)
            }
            if (s == cur) {
                placed = true;
                break;
            }
            if (lane == (s & 63)) ex_store(h, ex_pos(i, cur), s < 64 ? ka : kb, s < 64 ? ia : ib);  // child moves up into the hole
            cur = s;
        }
        const long long pc = ex_pos(i, cur);
        if (placed) {
            if (lane == 0) ex_store(h, pc, xk, xi);
            return;
        }
        i = pc;
    }
}
// heappush: new entry y at leaf position n (n = heap size before the push)
__device__ __forceinline__ void ex_push(const ExHeap& h, int n, u64 yk, u32 yi) {
    const int lane = threadIdx.x & 63;
    const long long np1 = (long long)n + 1;
    const long long qa = lane < 32 ? (np1 >> (lane + 1)) : 0;  // lane t: the ancestor t+1 levels above the leaf
    u64 ak = 0;
    u32 ai = 0;
    if (qa >= 1) ex_load(h, qa - 1, ak, ai);
    const u64 up = __ballot(qa >= 1 && yk < ak);                // smaller(child, parent): strict
    const int m = __ffsll((long long)~up) - 1;                  // the path is sorted: the larger ancestors are lanes 0 .. m-1
    if (lane < m) ex_store(h, (np1 >> lane) - 1, ak, ai);       // each moves one step down the path (lane 0's lands on the leaf)
    if (lane == 0) ex_store(h, (np1 >> m) - 1, yk, yi);
}

__global__ void ws_exact_reset_kernel(const uint8_t* __restrict__ mrk, const uint8_t* __restrict__ mask, int* __restrict__ out, int n,
                                      const int* __restrict__ flag) {
    if (*flag == 0) return;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x)
        if (!(mrk[p] && mask[p])) out[p] = 0;  // back to markers * mask: a marker pixel keeps its label through every flood
}

__global__ __launch_bounds__(64) void ws_exact_kernel(const float* __restrict__ inst, long long row_stride, int pix_stride,
                                                      const uint8_t* __restrict__ mask, int* out, u64* hkey, u32* hidx, int H, int W,
                                                      const int* __restrict__ flag) {
    if (*flag == 0) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_ex[];
    ExHeap h;
    h.sk = reinterpret_cast<volatile u64*>(s_ex);
    h.si = reinterpret_cast<volatile u32*>(s_ex + (size_t)EX_LDS * 8 + 8);
    h.gk = hkey;
    h.gi = hidx;
    const int lane = threadIdx.x & 63;
    const long long N = (long long)H * W;
    const double invW = 1.0 / (double)W;
    int n = 0;
    // ---- all marker pixels, raster order, age 0 (8 chunks of 64 pixels in flight) ----------------------------------------
    for (long long base = 0; base < N; base += 512) {
        int o[8];
        u32 kv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long long p = base + u * 64 + lane;
            o[u] = p < N ? out[p] : 0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long long p = base + u * 64 + lane;
            kv[u] = 0;
            if (o[u]) {
                int y, x;
                pix_yx(p, W, invW, y, x);
                kv[u] = order_key(-inst[y * row_stride + (long long)x * pix_stride]);
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            u64 m = __ballot(o[u] != 0);
            while (m) {
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                const u32 key = (u32)__builtin_amdgcn_readlane((int)kv[u], j);
                ex_push(h, n, (u64)key << 32, (u32)(base + u * 64 + j));
                ++n;
            }
        }
    }
    // ---- the flood -----------------------------------------------------------------------------------------------------------
    u32 age = 0;
    while (n > 0) {
        u64 rk;
        u32 ri;
        ex_load(h, 0, rk, ri);
        const u32 p = ex_uni(ri);
        const int y = (int)(p / (u32)W), x = (int)(p % (u32)W);
        // everything that only depends on the popped pixel / the heap size is requested first: the label, the four neighbour
        // probes and the last entry (which heappop moves to the root)
        const int lab = __hip_atomic_load(&out[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        --n;
        u64 xk = 0;
        u32 xi = 0;
        if (n > 0) ex_load(h, n, xk, xi);
        long long q = -1;
        if (lane == 0 && y > 0) q = (long long)p - W;
        if (lane == 1 && x > 0) q = (long long)p - 1;
        if (lane == 2 && x < W - 1) q = (long long)p + 1;
        if (lane == 3 && y < H - 1) q = (long long)p + W;
        uint8_t mq = 0;
        int oq = 1;
        float vq = 0.f;
        if (q >= 0) {
            mq = mask[q];
            oq = __hip_atomic_load(&out[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const int qy = (int)(q / W), qx = (int)(q % W);
            vq = -inst[qy * row_stride + (long long)qx * pix_stride];
        }
        if (n > 0) ex_sift_down(h, n, ex_uni64(xk), ex_uni(xi));
        const bool elig = q >= 0 && mq && oq == 0;
        if (elig) __hip_atomic_store(&out[q], lab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const u32 kq = order_key(vq);
        const u64 em = __ballot(elig);
#pragma unroll 1
        for (int t = 0; t < 4; ++t) {
            if (!((em >> t) & 1)) continue;
            ++age;
            const u32 qk = (u32)__builtin_amdgcn_readlane((int)kq, t);
            const u32 qi = (u32)__builtin_amdgcn_readlane((int)(u32)q, t);
            ex_push(h, n, ((u64)qk << 32) | age, qi);
            ++n;
        }
    }
}

extern "C" size_t cerb_pp_workspace_bytes(int h, int w) {
    const size_t n = (size_t)h * (size_t)w;
    return n * 96 + (4u << 20);
}

struct SideStreams {
    hipStream_t s[3];
    hipEvent_t fork, join[3];
};
static SideStreams* side_streams() {  // one set per device, created on first use (handles are used from one host thread, SURVEY par.8b)
    static SideStreams* per_dev[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!per_dev[dev]) {
        SideStreams* ss = new SideStreams();
        bool ok = hipEventCreateWithFlags(&ss->fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < 3 && ok; ++i)
            ok = hipStreamCreateWithFlags(&ss->s[i], hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&ss->join[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            delete ss;
            return nullptr;
        }
        per_dev[dev] = ss;
    }
    return per_dev[dev];
}

// exact_ties: literal skimage tie order for maps whose floods flag an ambiguous component -- a per-call argument (round 2 kept it in a
// process-wide flag that two host threads could race on).  The WSI band driver passes 0: the reference floods 4096^2 tiles there
// (infer/wsi.py:143-149), so the tie order of its heap is a property of ITS tiling.
extern "C" int cerb_postproc_nuclei(const float* inst, int H, int W, long long row_stride, int pix_stride, int32_t* labels_out,
                                    int32_t* n_inst_out, int32_t* n_ambiguous_out, int exact_ties, void* ws, size_t ws_bytes,
                                    void* hip_stream) {
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = pp_check_map("cerb_postproc_nuclei", inst && labels_out && ws, H, W, ws_bytes, cerb_pp_workspace_bytes(H, W))) return rc;
    const int n = H * W;
    Carve cv{(char*)ws, ws_bytes};
    int* LA = (int*)cv.take((size_t)n * 4);     // mask components
    int* areaA = (int*)cv.take((size_t)n * 4);
    int* LB = (int*)cv.take((size_t)n * 4);     // marker components (both colours until the markers are final)
    int* areaB = (int*)cv.take((size_t)n * 4);
    int* rank = (int*)cv.take((size_t)n * 4);   // the markers' border flags, then the LDS-heap tier list
    int* marker = (int*)cv.take((size_t)n * 4);
    int* hoff = (int*)cv.take((size_t)n * 4);
    int* hcnt = (int*)cv.take((size_t)n * 4);
    int* wl = (int*)cv.take((size_t)n * 4);
    u64* hkey = (u64*)cv.take((size_t)n * 8);
    u32* hidx = (u32*)cv.take((size_t)n * 4);
    CBox* cbox = (CBox*)cv.take((size_t)n * sizeof(CBox));
    uint8_t* msk0 = (uint8_t*)cv.take(n);
    uint8_t* msk = (uint8_t*)cv.take(n);
    uint8_t* mrk = (uint8_t*)cv.take(n);
    int* scantmp = (int*)cv.take((size_t)(n / SCAN_ITEMS + 4096) * 4 * 2);
    int* wl4 = (int*)cv.take((size_t)n * 4);    // tiny-window tier list
    int* lmax = (int*)cv.take((size_t)n * 4);   // per mask component: largest marker label
    const int nw = (n + 63) / 64;               // root bitmaps: one bit per pixel
    u64* bitsA = (u64*)cv.take((size_t)nw * 8); // kept mask components
    u64* bitsB = (u64*)cv.take((size_t)nw * 8); // final markers
    int* wpre = (int*)cv.take((size_t)nw * 4);  // roots before a bitmap word
    int* lmin = (int*)cv.take((size_t)n * 4);   // per mask component: smallest marker label
    int* tcnt = (int*)cv.take((size_t)pp_label_tiles(H, W) * 4);  // roots per labelling tile
    int* small = (int*)cv.take(256);  // [0]=any [1]=worklist count [2]=n_inst scratch [3]=ambiguous scratch [8..12]=tier counts [16]=heap total
    if (!small) return cerb_set_error("cerb_postproc_nuclei: workspace carve failed");
    const unsigned g = grid_for(n);
    // Four pixels per thread want whole quads per row and 16-byte aligned maps (the workspace arrays are 256-byte aligned); every other map takes the
    // one-pixel-per-thread passes, and CERB_PP_ONE_PIXEL_THREADS (developers' build) sends any map through them so that a test can hold both to the same bytes.
    static const bool narrow = cerb_dev_getenv("CERB_PP_ONE_PIXEL_THREADS") != nullptr;
    const bool wide = !narrow && W % 4 == 0 && (uintptr_t)labels_out % 16 == 0;

    PP_OK(hipMemsetAsync(small, 0, 256, st));
    // (A) mask: erode -> label -> drop components < 8 px   (postproc.py:365-368)
    // (round 5 tried threshold + erosion + tile labelling as ONE kernel over a 66 x 34 window per tile: bit-exact, 0.68 ms against 0.51 ms for the three
    // launches below -- the 8-byte loads, the divergent halo columns and three barriers per tile cost more than the two byte planes it saved)
    if (W % 4 == 0 && ((uintptr_t)msk0 | (uintptr_t)msk | (uintptr_t)mrk) % 4 == 0) {  // (these two touch workspace maps only: `labels_out` does not matter to them)
        const unsigned g4 = grid_for(n / 4);
        const bool packed = pix_stride == 2 && row_stride % 4 == 0 && (uintptr_t)inst % 16 == 0;
        hipLaunchKernelGGL(packed ? nuc_threshold4_kernel<true> : nuc_threshold4_kernel<false>, dim3(g4), dim3(256), 0, st, inst, row_stride, pix_stride, H, W,
                           (uint32_t*)msk0, (uint32_t*)mrk, small);
        hipLaunchKernelGGL(erode_cross4_kernel, dim3(g4), dim3(256), 0, st, (const uint32_t*)msk0, (uint32_t*)msk, H, W);
    } else {
        hipLaunchKernelGGL(nuc_threshold_kernel, dim3(g), dim3(256), 0, st, inst, row_stride, pix_stride, H, W, msk0, mrk, small);
        hipLaunchKernelGGL(erode_cross_kernel, dim3(g), dim3(256), 0, st, msk0, msk, H, W);
    }
    // round 6: the tile labellings leave their border columns in a compact array (2 x (tiles_x - 1) x H ints: wl4 is free until the flood work lists) and the
    // seam passes read their vertical seams from it
    int* seam_cols = wl4;
    // (the root list of the wide form: hoff is free until roots_setup_kernel; its roots per tile: tcnt)
    if (pp_label_mask_min_area(msk, LA, areaA, 8, H, W, st, bitsA, wide, hoff, tcnt, seam_cols)) return 1;
    // (B) markers: inner > 0.5 -> label -> drop < 4 px -> fill holes -> label (postproc.py:370-377)
    // (rank: free until the flood work lists, serves as the border flags; marker: free until the flood work lists, holds the root list)
    if (pp_markers_two_colour(mrk, LB, areaB, rank, marker, tcnt, 4, H, W, st, bitsB, wide, seam_cols)) return 1;
    // (C) per-component state and heap ranges from the mask's root bitmap, before the pass that fills in the label extremes
    int* unl = areaB;  // free again: per-root count of unlabelled mask pixels
    int* wl3 = marker; // big-window tier list
    hipLaunchKernelGGL(roots_setup_kernel, dim3(nblk(nw, 256)), dim3(256), 0, st, bitsA, nw, areaA, hoff, hcnt, unl, lmin, lmax, cbox, H, W, small + 16);
    KCHECK();
    // marker ids = 1 + rank of the component's root among all roots (scipy's label order), written straight into the watershed's start map
    const int* boff = nullptr;
    if (pp_scan_exclusive_popc(bitsB, wpre, nw, scantmp, st, &boff, n_inst_out, small)) return 1;
    if (wide) hipLaunchKernelGGL(nuc_marker_out4_kernel, dim3(grid_for(n / 4)), dim3(256), 0, st, (const int4*)LB, bitsB, wpre, boff, (const uint32_t*)msk, (int4*)labels_out,
                                 (long long)n / 4, (const int4*)LA, lmin, lmax, (const uint32_t*)mrk);
    else hipLaunchKernelGGL(nuc_marker_out_bits_kernel, dim3(g), dim3(256), 0, st, LB, bitsB, wpre, boff, msk, labels_out, n, LA, lmin, lmax);
    // (D) watershed(-inner, marker, mask)   (postproc.py:378): seeds, floodable-pixel counts and boxes of the components that reach a flood
    if (wide) {
        hipLaunchKernelGGL(ws_seed_bbox4_kernel, dim3(grid_for(n / 4)), dim3(256), 0, st, inst, row_stride, pix_stride, (const uint32_t*)msk, (const int4*)labels_out,
                           (const int4*)LA, hoff, hcnt, hkey, hidx, H, W, unl, lmin, lmax, cbox);
    } else {
        hipLaunchKernelGGL(ws_seed_kernel, dim3(g), dim3(256), 0, st, inst, row_stride, pix_stride, msk, labels_out, LA, hoff, hcnt, hkey, hidx, H, W, unl,
                           lmin, lmax);
        hipLaunchKernelGGL(ws_bbox_kernel, dim3(g), dim3(256), 0, st, LA, msk, cbox, H, W, lmin, lmax);
    }
    // (E) work lists, one per flood tier
    int* counts = small + 8;  // [0] window tier, [1] LDS-heap tier, [2] global tier
    hipLaunchKernelGGL(ws_worklist_bits_kernel, dim3(nblk(nw, 256) < 4096 ? nblk(nw, 256) : 4096), dim3(256), 0, st, bitsA, nw, hcnt, areaA, unl, cbox, lmin, lmax, wl, rank, wl3, wl4, counts, n);
    // (F) floods
    {
        auto k_tiny = ws_flood_window_kernel<WS_TINY_WIN, WS_TINY_CAP, 4>;
        auto k_small = ws_flood_window_kernel<WS_WIN_CAP, WS_LDS_CAP, 2>;
        auto k_big = ws_flood_window_kernel<WS_BIGWIN_CAP, WS_BIGHEAP_CAP, 1>;
        constexpr int lds_small = 2 * (WS_LDS_CAP * 10 + WS_WIN_CAP * 8), lds_big = WS_BIGHEAP_CAP * 10 + WS_BIGWIN_CAP * 8;
        constexpr int lds_tiny = 4 * (WS_TINY_CAP * 10 + WS_TINY_WIN * 8);
        static bool attr_done[64] = {};
        if (cerb_attr_needed(attr_done)) {
            PP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_small), hipFuncAttributeMaxDynamicSharedMemorySize, lds_small));
            PP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tiny), hipFuncAttributeMaxDynamicSharedMemorySize, lds_tiny));
            PP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_big), hipFuncAttributeMaxDynamicSharedMemorySize, lds_big));
        }
        // The tiers touch disjoint components and each one ends with the tail of its longest flood: fork them onto side streams
        // (created once per device) so that the tails overlap instead of adding up; `st` resumes when all of them are done.
        SideStreams* ss = side_streams();
        if (!ss) return cerb_set_error("cerb_postproc_nuclei: side stream creation failed");
        if (cerb_dev_getenv("CERB_PP_DEBUG_COUNTS")) {  // developer probe: components per flood tier
            int hc[8] = {};
            PP_OK(hipStreamSynchronize(st));
            PP_OK(hipMemcpy(hc, counts, sizeof(hc), hipMemcpyDeviceToHost));
            fprintf(stderr, "flood tiers: small-window %d, lds-heap %d, global-heap %d, big-window %d, tiny-window %d\n", hc[0], hc[1], hc[2], hc[3], hc[4]);
        }
        static const bool serial_floods = cerb_dev_getenv("CERB_PP_SERIAL_FLOODS") != nullptr;  // developer probe: the tiers one after the other on `st`
        SideStreams serial_ss;
        if (serial_floods) {
            serial_ss = *ss;
            serial_ss.s[0] = serial_ss.s[1] = serial_ss.s[2] = st;
            ss = &serial_ss;
        }
        PP_OK(hipEventRecord(ss->fork, st));
        for (int i = 0; i < 3; ++i) PP_OK(hipStreamWaitEvent(ss->s[i], ss->fork, 0));
        hipLaunchKernelGGL(k_tiny, dim3(256 * 3), dim3(256), lds_tiny, ss->s[0], inst, row_stride, pix_stride, msk, LA, labels_out, wl4, counts + 4, cbox,
                           H, W, small + 3, small + 24);
        hipLaunchKernelGGL(k_small, dim3(256 * 2), dim3(128), lds_small, ss->s[1], inst, row_stride, pix_stride, msk, LA, labels_out, wl, counts + 0, cbox,
                           H, W, small + 3, small + 25);
        // (launching this tier FIRST -- its longest flood is the critical path -- measured worse: its 151-KB workgroups then keep the other tiers off
        // every CU that holds one; behind them it starts where they have left)
        hipLaunchKernelGGL(k_big, dim3(256), dim3(64), lds_big, st, inst, row_stride, pix_stride, msk, LA, labels_out, wl3, counts + 3, cbox, H, W,
                           small + 3, small + 26);
        // the fill of the single-label components (isolated nuclei: no flood) touches other pixels than any flood: beside them, not before them
        if (wide) hipLaunchKernelGGL(ws_fill_single4_kernel, dim3(grid_for(n / 4)), dim3(256), 0, ss->s[2], (const uint32_t*)msk, (const int4*)LA, lmin, lmax, (int4*)labels_out, (long long)n / 4);
        else hipLaunchKernelGGL(ws_fill_single_kernel, dim3(g), dim3(256), 0, ss->s[2], msk, LA, lmin, lmax, labels_out, n);
        hipLaunchKernelGGL(ws_flood_lds_kernel, dim3(256 * 2), dim3(256), 0, ss->s[2], inst, row_stride, pix_stride, msk, labels_out, rank, counts + 1,
                           hoff, hcnt, hkey, hidx, H, W, small + 3, small + 27);
        hipLaunchKernelGGL(ws_flood_kernel, dim3(256 * 4), dim3(256), 0, ss->s[2], inst, row_stride, pix_stride, msk, labels_out, wl, counts + 2, hoff,
                           hcnt, hkey, hidx, H, W, small + 3, n, small + 28);
        for (int i = 0; i < 3; ++i) {
            PP_OK(hipEventRecord(ss->join[i], ss->s[i]));
            PP_OK(hipStreamWaitEvent(st, ss->join[i], 0));
        }
    }
    KCHECK();
    if (exact_ties) {
        // (G) exact replay.  Components whose result depends on skimage's heap-layout order between equal-valued markers were counted in small[3]:
        // when there is one, the whole map is re-flooded through the literal emulation of that heap (both kernels return at once
        // when the count is zero -- no host round trip decides this).
        constexpr int lds_exact = EX_LDS * 8 + 8 + EX_LDS * 4 + 4;
        static bool attr_done2[64] = {};
        if (cerb_attr_needed(attr_done2))
            PP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(ws_exact_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_exact));
        hipLaunchKernelGGL(ws_exact_reset_kernel, dim3(g), dim3(256), 0, st, mrk, msk, labels_out, n, small + 3);
        hipLaunchKernelGGL(ws_exact_kernel, dim3(1), dim3(64), lds_exact, st, inst, row_stride, pix_stride, msk, labels_out, hkey, hidx, H, W, small + 3);
        KCHECK();
    }
    if (n_ambiguous_out) PP_OK(hipMemcpyAsync(n_ambiguous_out, small + 3, 4, hipMemcpyDeviceToDevice, st));
    return 0;
}
