// The gland / lumen / eroded-map stage of the instance post-processing on gfx950 (overview: pp_nuclei.hip; labelling: pp_label.hip through the
// launchers of pp_common.h): threshold -> label, drop small components -> per instance crop -> dilate -> fill holes -> paste.
#include <cmath>
#include <cstdlib>

#include "pp_common.h"

// =================================================================================================================
// Gland / lumen: threshold, per-instance crop -> dilate -> fill holes -> paste
// =================================================================================================================
__global__ void gl_threshold_kernel(const float* __restrict__ inst, long long row_stride, int pix_stride, int H, int W, float thr,
                                    uint8_t* __restrict__ fg) {
    const long long n = (long long)H * W;
    const double invW = 1.0 / (double)W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        int y, x;
        pix_yx(p, W, invW, y, x);
        const float* s = inst + y * row_stride + (long long)x * pix_stride;
        const float c = s[1] > 0.5f ? 1.f : 0.f;  // inst_cnt binarised (postproc.py:280-282)
        fg[p] = (s[0] - c) > thr;
    }
}
// PostProcInstErodedMap (loader/postproc.py:147-242): the map is the ONE inner-probability channel of a two-class INST head, fg = inner > 0.5
__global__ void er_threshold_kernel(const float* __restrict__ inner, long long row_stride, int pix_stride, int H, int W, uint8_t* __restrict__ fg) {
    const long long n = (long long)H * W;
    const double invW = 1.0 / (double)W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        int y, x;
        pix_yx(p, W, invW, y, x);
        fg[p] = inner[y * row_stride + (long long)x * pix_stride] > 0.5f;
    }
}
struct Box {
    int y1, y2, x1, x2;
};
__global__ void box_init_kernel(Box* b, int n, int H, int W) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        b[i].y1 = H;
        b[i].x1 = W;
        b[i].y2 = 0;
        b[i].x2 = 0;
    }
}
__global__ void box_accum_kernel(const int* __restrict__ lab, Box* b, int H, int W) {
    const long long n = (long long)H * W;
    const double invW = 1.0 / (double)W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        const int l = lab[p];
        if (!l) continue;
        int y, x;
        pix_yx(p, W, invW, y, x);
        // only pixels on the instance outline can be bounding-box extremes (keeps the atomics off the interior)
        if (y > 0 && y < H - 1 && x > 0 && x < W - 1 && lab[p - W] == l && lab[p + W] == l && lab[p - 1] == l && lab[p + 1] == l) continue;
        // the extremes only ever move outwards, so a (possibly stale) plain read that already covers this pixel makes the atomic
        // unnecessary -- a slide-sized ragged instance would otherwise serialise millions of atomics on one box
        const volatile Box* vb = b + l;
        if (y < vb->y1) atomicMin(&b[l].y1, y);
        if (y + 1 > vb->y2) atomicMax(&b[l].y2, y + 1);
        if (x < vb->x1) atomicMin(&b[l].x1, x);
        if (x + 1 > vb->x2) atomicMax(&b[l].x2, x + 1);
    }
}
// crop = bounding box padded by 2*ksize on each side only where the padded edge stays inside (postproc.py:296-300)
__global__ void box_pad_kernel(Box* b, int* __restrict__ area, int n_inst, int H, int W, int pad) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= n_inst; i += gridDim.x * blockDim.x) {
        if (i == 0) {
            area[0] = 0;
            continue;
        }
        Box c = b[i];
        c.y1 = c.y1 - pad >= 0 ? c.y1 - pad : c.y1;
        c.x1 = c.x1 - pad >= 0 ? c.x1 - pad : c.x1;
        c.x2 = c.x2 + pad <= W - 1 ? c.x2 + pad : c.x2;
        c.y2 = c.y2 + pad <= H - 1 ? c.y2 + pad : c.y2;
        b[i] = c;
        area[i] = (c.y2 - c.y1) * (c.x2 - c.x1);
    }
}
struct Spans {
    int k, a;
    int j1[32], j2[32];
};
// The crops of a batch are laid out back to back (crop-local row-major); the kernels below run over that flat element
// space so large and small instances share the machine.  coff[id] = start of instance id's crop; element e belongs to the
// last instance whose start is <= e.
__device__ __forceinline__ int find_inst(const int* __restrict__ coff, int first, int cnt, int e_abs) {
    int lo = first, hi = first + cnt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (coff[mid] <= e_abs) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// dilation of (lab == id) by the ellipse, clipped to the crop (cv2.dilate on the crop; the border never wins the max)
__global__ __launch_bounds__(256) void gl_dilate_kernel(const int* __restrict__ lab, const Box* __restrict__ box, const int* __restrict__ coff,
                                                        int first, int cnt, int tot, int W, Spans se, uint8_t* __restrict__ dil) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += gridDim.x * blockDim.x) {
        const int id = find_inst(coff, first, cnt, e + coff[first]);
        const Box c = box[id];
        const int ch = c.y2 - c.y1, cw = c.x2 - c.x1;
        const int i = e - (coff[id] - coff[first]);
        const int y = i / cw, x = i % cw;
        uint8_t v = 0;
        for (int r = 0; r < se.k && !v; ++r) {
            const int yy = y + r - se.a;
            if (yy < 0 || yy >= ch) continue;
            const int xa = max(x + se.j1[r] - se.a, 0), xb = min(x + se.j2[r] - se.a, cw);
            const int* row = lab + (long long)(c.y1 + yy) * W + c.x1;
            for (int xx = xa; xx < xb; ++xx)
                if (row[xx] == id) {
                    v = 1;
                    break;
                }
        }
        dil[e] = v;
    }
}
// background CCL inside every crop of the batch (crop-local 4-connectivity, shared union-find array)
__global__ __launch_bounds__(256) void gl_bg_init_kernel(const uint8_t* __restrict__ dil, int tot, int* __restrict__ L, int* __restrict__ border) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += gridDim.x * blockDim.x) {
        L[e] = dil[e] ? -1 : e;
        border[e] = 0;
    }
}
__global__ __launch_bounds__(256) void gl_bg_merge_kernel(const uint8_t* __restrict__ dil, const Box* __restrict__ box, const int* __restrict__ coff,
                                                          int first, int cnt, int tot, int* L) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += gridDim.x * blockDim.x) {
        if (dil[e]) continue;
        const int id = find_inst(coff, first, cnt, e + coff[first]);
        const Box c = box[id];
        const int cw = c.x2 - c.x1;
        const int i = e - (coff[id] - coff[first]);
        const int x = i % cw;
        const bool left = x > 0 && !dil[e - 1];
        if (i >= cw && !dil[e - cw]) {
            // one union per pair of vertically adjacent background runs: at the first column where they overlap either the lower run starts here, or the upper one does
            const bool up_starts = !(x > 0 && !dil[e - cw - 1]);
            if (!left || up_starts) uf_union(L, e, e - cw);
        }
        if (left) uf_union(L, e, e - 1);
    }
}
__global__ __launch_bounds__(256) void gl_bg_border_kernel(const Box* __restrict__ box, const int* __restrict__ coff, int first, int cnt, int tot,
                                                           int* L, int* __restrict__ border) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += gridDim.x * blockDim.x) {
        if (L[e] < 0) continue;
        const int r = uf_find(L, e);
        L[e] = r;
        const int id = find_inst(coff, first, cnt, e + coff[first]);
        const Box c = box[id];
        const int ch = c.y2 - c.y1, cw = c.x2 - c.x1;
        const int i = e - (coff[id] - coff[first]);
        const int y = i / cw, x = i % cw;
        if (y == 0 || y == ch - 1 || x == 0 || x == cw - 1) border[r] = 1;
    }
}
__global__ __launch_bounds__(256) void gl_paste_kernel(const uint8_t* __restrict__ dil, const Box* __restrict__ box, const int* __restrict__ coff,
                                                       int first, int cnt, int tot, const int* __restrict__ L, const int* __restrict__ border, int W,
                                                       int* __restrict__ out) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += gridDim.x * blockDim.x) {
        bool in = dil[e];
        if (!in) in = !border[L[e]];  // hole of the dilated instance inside its crop
        if (!in) continue;
        const int id = find_inst(coff, first, cnt, e + coff[first]);
        const Box c = box[id];
        const int cw = c.x2 - c.x1;
        const int i = e - (coff[id] - coff[first]);
        atomicMax(&out[(long long)(c.y1 + i / cw) * W + c.x1 + i % cw], id);  // ids ascend: later id overwrites
    }
}
__global__ void mask_lumen_kernel(int* __restrict__ lumen, const int* __restrict__ gland, long long n) {
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x)
        if (gland[p] <= 0) lumen[p] = 0;
}

static void ellipse_spans(int k, Spans* s) {  // cv2.getStructuringElement(MORPH_ELLIPSE, (k,k)) row spans
    s->k = k;
    s->a = k / 2;
    const int r = k / 2, c = k / 2;
    const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
    for (int i = 0; i < k; ++i) {
        const int dy = i - r;
        s->j1[i] = s->j2[i] = 0;
        if (abs(dy) <= r) {
            const int dx = (int)lrint(c * sqrt((r * r - dy * dy) * inv_r2));
            s->j1[i] = c - dx > 0 ? c - dx : 0;
            s->j2[i] = c + dx + 1 < k ? c + dx + 1 : k;
        }
    }
}

// one_channel: the eroded-map scheme (cerb_postproc_eroded) -- `inst` holds the inner probability alone and `thr` is not used
static int gland_lumen(const float* inst, int H, int W, long long row_stride, int pix_stride, float thr, int min_size, int ksize,
                       int32_t* labels_out, int32_t* n_inst_out, void* ws, size_t ws_bytes, hipStream_t st, const char* who, bool one_channel = false) {
    if (int rc = pp_check_map(who, inst && labels_out && ws, H, W, ws_bytes, cerb_pp_workspace_bytes(H, W))) return rc;
    if (ksize < 1 || ksize > 32) return cerb_set_error(std::string(who) + ": structuring element size out of range (ds_factor too small/large)");
    const int n = H * W;
    Carve cv{(char*)ws, ws_bytes};
    int* L = (int*)cv.take((size_t)n * 4);
    int* area = (int*)cv.take((size_t)n * 4);
    int* flag = (int*)cv.take((size_t)n * 4);
    int* rank = (int*)cv.take((size_t)n * 4);
    int* lab = (int*)cv.take((size_t)n * 4);
    uint8_t* fg = (uint8_t*)cv.take(n);
    int* scantmp = (int*)cv.take((size_t)(n / SCAN_ITEMS + 4096) * 4 * 2);
    int* small = (int*)cv.take(256);
    // per-instance tables: at most n / max(min_size,1) + 1 instances
    const int max_inst = n / (min_size > 0 ? min_size : 1) + 2;
    Box* box = (Box*)cv.take((size_t)max_inst * sizeof(Box));
    int* carea = (int*)cv.take((size_t)max_inst * 4);
    int* coff = (int*)cv.take((size_t)max_inst * 4);
    int* scantmp2 = (int*)cv.take((size_t)(max_inst / SCAN_ITEMS + 4096) * 4 * 2);
    if (!scantmp2) return cerb_set_error(std::string(who) + ": workspace carve failed");
    // the rest of the workspace holds the crops of one batch: 1 (dil) + 4 (L) + 4 (border) bytes per crop pixel
    const size_t crop_cap = cv.left / 10 > 256 ? (cv.left - 4096) / 10 : 0;
    uint8_t* dil = (uint8_t*)cv.take(crop_cap);
    int* cL = (int*)cv.take(crop_cap * 4);
    int* cB = (int*)cv.take(crop_cap * 4);
    if (!cB) return cerb_set_error(std::string(who) + ": workspace carve failed");
    const unsigned g = grid_for(n);

    if (one_channel) hipLaunchKernelGGL(er_threshold_kernel, dim3(g), dim3(256), 0, st, inst, row_stride, pix_stride, H, W, fg);
    else hipLaunchKernelGGL(gl_threshold_kernel, dim3(g), dim3(256), 0, st, inst, row_stride, pix_stride, H, W, thr, fg);
    if (pp_label_ranked(fg, L, area, min_size, flag, rank, scantmp, lab, small, H, W, st)) return 1;
    PP_OK(hipMemsetAsync(labels_out, 0, (size_t)n * 4, st));
    int n_inst = 0;  // the one host round trip of this path: 4 bytes of metadata (number of instances)
    PP_OK(hipMemcpyAsync(&n_inst, small, 4, hipMemcpyDeviceToHost, st));
    int area0 = 0;   // pixels of the component rooted at pixel 0 (a component's root is its first pixel in raster order)
    if (one_channel) PP_OK(hipMemcpyAsync(&area0, area, 4, hipMemcpyDeviceToHost, st));
    PP_OK(hipStreamSynchronize(st));
    if (one_channel && area0 == n) {
        // PostProcInstErodedMap walks `np.unique(inst_lab).tolist()[1:]` (loader/postproc.py:160): the smallest label is dropped as "the background".  A map
        // without one background pixel is one component with id 1 -- that id is what gets dropped, and the reference returns an empty map.
        n_inst = 0;
        PP_OK(hipMemsetAsync(small, 0, 4, st));
    }
    if (n_inst_out) PP_OK(hipMemcpyAsync(n_inst_out, small, 4, hipMemcpyDeviceToDevice, st));
    if (n_inst == 0) return 0;
    if (n_inst + 1 > max_inst) return cerb_set_error(std::string(who) + ": internal: instance table overflow");
    hipLaunchKernelGGL(box_init_kernel, dim3(nblk(n_inst + 1, 256)), dim3(256), 0, st, box, n_inst + 1, H, W);
    hipLaunchKernelGGL(box_accum_kernel, dim3(g), dim3(256), 0, st, lab, box, H, W);
    hipLaunchKernelGGL(box_pad_kernel, dim3(nblk(n_inst + 1, 256)), dim3(256), 0, st, box, carea, n_inst, H, W, ksize * 2);
    if (pp_scan_exclusive(carea, coff, n_inst + 1, scantmp2, st)) return 1;
    KCHECK();
    // batch instances so that the crops of a batch fit the crop workspace (needs the crop areas on the host)
    int* h_area = (int*)malloc((size_t)(n_inst + 2) * 4);
    PP_OK(hipMemcpyAsync(h_area, carea, (size_t)(n_inst + 1) * 4, hipMemcpyDeviceToHost, st));
    PP_OK(hipStreamSynchronize(st));
    Spans se;
    ellipse_spans(ksize, &se);
    int first = 1, rc = 0;
    // coff is a 32-bit running sum over ALL crops (the kernels index a batch relative to coff[first]): thousands of small instances with a padded
    // box each (nuclei at min_size 8) must still fit it
    long long crop_sum = 0;
    for (int i = 1; i <= n_inst; ++i) crop_sum += (long long)h_area[i];
    if (crop_sum >= (1ll << 31)) {
        rc = cerb_set_error(std::string(who) + ": the instance crops of this map add up to 2^31 pixels or more");
        first = n_inst + 1;
    }
    while (first <= n_inst) {
        int last = first;
        size_t tot = (size_t)h_area[first];
        if (tot > crop_cap || tot >= (1ull << 31)) {
            rc = cerb_set_error(std::string(who) + ": one instance crop exceeds the workspace");
            break;
        }
        while (last + 1 <= n_inst && tot + (size_t)h_area[last + 1] <= crop_cap && tot + (size_t)h_area[last + 1] < (1ull << 31)) tot += (size_t)h_area[++last];
        const int cnt = last - first + 1;
        const int tot_i = (int)tot;
        const unsigned gb = grid_for(tot_i);
        hipLaunchKernelGGL(gl_dilate_kernel, dim3(gb), dim3(256), 0, st, lab, box, coff, first, cnt, tot_i, W, se, dil);
        hipLaunchKernelGGL(gl_bg_init_kernel, dim3(gb), dim3(256), 0, st, dil, tot_i, cL, cB);
        hipLaunchKernelGGL(gl_bg_merge_kernel, dim3(gb), dim3(256), 0, st, dil, box, coff, first, cnt, tot_i, cL);
        hipLaunchKernelGGL(gl_bg_border_kernel, dim3(gb), dim3(256), 0, st, box, coff, first, cnt, tot_i, cL, cB);
        hipLaunchKernelGGL(gl_paste_kernel, dim3(gb), dim3(256), 0, st, dil, box, coff, first, cnt, tot_i, cL, cB, W, labels_out);
        first = last + 1;
    }
    free(h_area);
    if (rc) return rc;
    KCHECK();
    return 0;
}

extern "C" int cerb_postproc_gland(const float* inst, int H, int W, long long row_stride, int pix_stride, float ds, int32_t* labels_out,
                                   int32_t* n_inst_out, void* ws, size_t ws_bytes, void* hip_stream) {
    // python: ksize = int((11-1)*ds); min_size = int(1000*(ds**2))   (postproc.py:272-274,287)
    return gland_lumen(inst, H, W, row_stride, pix_stride, 0.55f, (int)(1000.0 * ((double)ds * (double)ds)), (int)(10.0 * (double)ds), labels_out,
                       n_inst_out, ws, ws_bytes, (hipStream_t)hip_stream, "cerb_postproc_gland");
}
extern "C" int cerb_postproc_lumen(const float* inst, int H, int W, long long row_stride, int pix_stride, float ds, int32_t* labels_out,
                                   int32_t* n_inst_out, void* ws, size_t ws_bytes, void* hip_stream) {
    return gland_lumen(inst, H, W, row_stride, pix_stride, 0.5f, (int)(150.0 * ((double)ds * (double)ds)), (int)(2.0 * (double)ds), labels_out,
                       n_inst_out, ws, ws_bytes, (hipStream_t)hip_stream, "cerb_postproc_lumen");
}
// PostProcInstErodedMap (loader/postproc.py:147-265, the IP-ERODED-3 / -11 codes): threshold 0.5 on the inner map, remove_small_objects, then the gland
// scheme above for all three tissues -- nuclei included, with the 3 x 3 element.  No ds_factor: the reference's `scale` argument is never read.
extern "C" int cerb_postproc_eroded(const float* inner, int H, int W, long long row_stride, int pix_stride, int tissue, int32_t* labels_out,
                                    int32_t* n_inst_out, void* ws, size_t ws_bytes, void* hip_stream) {
    static const int min_size[3] = {1500, 150, 8}, ksize[3] = {11, 3, 3};  // Gland, Lumen, Nuclei (postproc.py:151-156, :183-188, :215-220)
    if (tissue < 0 || tissue > 2) return cerb_set_error("cerb_postproc_eroded: tissue must be 0 (Gland), 1 (Lumen) or 2 (Nuclei)");
    return gland_lumen(inner, H, W, row_stride, pix_stride, 0.5f, min_size[tissue], ksize[tissue], labels_out, n_inst_out, ws, ws_bytes,
                       (hipStream_t)hip_stream, "cerb_postproc_eroded", true);
}
extern "C" int cerb_mask_lumen_by_gland(int32_t* lumen, const int32_t* gland, long long n_pix, void* hip_stream) {
    if (!lumen || !gland || n_pix < 0) return cerb_set_error("cerb_mask_lumen_by_gland: bad arguments");
    hipLaunchKernelGGL(mask_lumen_kernel, dim3(grid_for(n_pix)), dim3(256), 0, (hipStream_t)hip_stream, lumen, gland, n_pix);
    KCHECK();
    return 0;
}
