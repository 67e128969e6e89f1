// Training augmentations on the device (include/cerberus_hip.h, section "training augmentations"; cerberus_amd/augs.py): the affine warp + centre crop +
// flips of image and annotation in one gather, Gaussian / median blur, Gaussian noise, the four colour operations and the channel sums behind contrast.
//
// The host draws every random number; each kernel is a pure function of (input, per-sample parameters) and processes the whole batch in one launch:
// grid = (pixel groups of one sample, samples), so a sample's parameters are uniform over a workgroup and a sample that is skipped costs one early exit.
// Stencil kernels (warp, blurs) take one thread per output pixel; the point-wise kernels (noise, colour, sums) take four consecutive pixels per thread,
// 12 bytes moved as three dwords where the sample's base is 4-byte aligned.  Every byte offset is 64-bit and nothing outside the stated shapes is touched.
// All of these passes are bound by memory traffic of a few MB per batch; none uses LDS, none loops persistently.
//
// This file is compiled with floating-point contraction OFF (cerberus_amd/build.py: EXTRA_FLAGS): the header defines every fp64 result as separately rounded
// products and sums (what numpy does), and a fused multiply-add would round once where the definition rounds twice.
#include "cerb_net.h"

namespace {

constexpr int AUG_BLOCK = 256;
constexpr int AUG_MAX_SIDE = 16384;
constexpr int AUG_MAX_N = 65535;       // samples go to gridDim.y
constexpr int AUG_SUM_ITERS = 8;       // pixel groups per thread in the channel-sum pass
typedef unsigned long long u64;

// ---- four pixels (12 bytes) of one sample ----------------------------------------------------------------------------------------------------------
// p: the sample's first byte; g: pixel group (pixels 4 g .. 4 g + 3); npx: pixels of the sample.  Returns the number of valid pixels (0 .. 4).
__device__ __forceinline__ int aug_load4(const uint8_t* __restrict__ p, long long g, long long npx, bool vec, uint8_t b[12]) {
    const long long first = g * 4;
    if (first >= npx) return 0;
    const int cnt = (int)(npx - first < 4 ? npx - first : 4);
    if (vec && cnt == 4) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p + first * 3);
        const uint32_t a0 = q[0], a1 = q[1], a2 = q[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = (uint8_t)(a0 >> (8 * i)), b[4 + i] = (uint8_t)(a1 >> (8 * i)), b[8 + i] = (uint8_t)(a2 >> (8 * i));
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) b[i] = i < cnt * 3 ? p[first * 3 + i] : (uint8_t)0;
    }
    return cnt;
}
__device__ __forceinline__ void aug_store4(uint8_t* __restrict__ p, long long g, int cnt, bool vec, const uint8_t b[12]) {
    const long long first = g * 4;
    if (vec && cnt == 4) {
        uint32_t a[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) a[j] = (uint32_t)b[4 * j] | ((uint32_t)b[4 * j + 1] << 8) | ((uint32_t)b[4 * j + 2] << 16) | ((uint32_t)b[4 * j + 3] << 24);
        uint32_t* q = reinterpret_cast<uint32_t*>(p + first * 3);
        q[0] = a[0], q[1] = a[1], q[2] = a[2];
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i)
            if (i < cnt * 3) p[first * 3 + i] = b[i];
    }
}
__device__ __forceinline__ uint8_t aug_clip_trunc(double x) {  // trunc(clip(x, 0, 255)) of a finite x
    x = x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x);
    return (uint8_t)(int)x;
}
__device__ __forceinline__ bool aug_finite(double v) { return v == v && v - v == 0.0; }

// ---- warp ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_BLOCK) void aug_warp_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ ann, int H, int W, int C,
                                                             const long long* __restrict__ maps, uint8_t* __restrict__ img_out,
                                                             int32_t* __restrict__ ann_out, int h, int w) {
    const long long npx = (long long)h * w, pix = (long long)blockIdx.x * AUG_BLOCK + threadIdx.x;
    if (pix >= npx) return;
    const int s = blockIdx.y;
    const int v = (int)(pix / w), u = (int)(pix - (long long)v * w);
    const long long* m = maps + (long long)s * 6;
    // (unsigned products wrap instead of overflowing on a nonsensical map; the range test below is what keeps every read inside the source)
    const long long xs = (long long)((u64)m[0] * (u64)u + (u64)m[1] * (u64)v + (u64)m[2] + 32768ull) >> 16;
    const long long ys = (long long)((u64)m[3] * (u64)u + (u64)m[4] * (u64)v + (u64)m[5] + 32768ull) >> 16;
    const bool in = xs >= 0 && xs < W && ys >= 0 && ys < H;
    const long long so = ((long long)s * H + (in ? ys : 0)) * W + (in ? xs : 0), d = (long long)s * npx + pix;
    if (img != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) img_out[d * 3 + c] = in ? img[so * 3 + c] : (uint8_t)0;
    }
    if (ann != nullptr) {
        for (int c = 0; c < C; ++c) ann_out[d * C + c] = in ? ann[so * C + c] : 0;
    }
}

// ---- Gaussian blur ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int aug_gauss_w(int k, int i) {  // [1], [1 2 1], [1 4 6 4 1]
    if (k == 5) return i == 2 ? 6 : ((i == 1 || i == 3) ? 4 : 1);
    if (k == 3) return i == 1 ? 2 : 1;
    return 1;
}
__device__ __forceinline__ bool aug_ksize_ok(int k) { return k == 1 || k == 3 || k == 5; }

__global__ __launch_bounds__(AUG_BLOCK) void aug_gauss_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int w,
                                                              const int32_t* __restrict__ kxs, const int32_t* __restrict__ kys) {
    const int s = blockIdx.y;
    const int kx = kxs[s], ky = kys[s];
    if (!aug_ksize_ok(kx) || !aug_ksize_ok(ky)) return;  // 0 (or anything else): the sample is not written
    const long long npx = (long long)h * w, pix = (long long)blockIdx.x * AUG_BLOCK + threadIdx.x;
    if (pix >= npx) return;
    const int y = (int)(pix / w), x = (int)(pix - (long long)y * w);
    const uint8_t* sp = src + (long long)s * npx * 3;
    const int rx = kx >> 1, ry = ky >> 1, shift = 2 * (rx + ry);
    int acc[3] = {0, 0, 0};
    for (int dy = 0; dy < ky; ++dy) {
        const int yy = min(max(y + dy - ry, 0), h - 1), wy = aug_gauss_w(ky, dy);
        for (int dx = 0; dx < kx; ++dx) {
            const int xx = min(max(x + dx - rx, 0), w - 1), wt = wy * aug_gauss_w(kx, dx);
            const uint8_t* q = sp + ((long long)yy * w + xx) * 3;
            acc[0] += wt * q[0], acc[1] += wt * q[1], acc[2] += wt * q[2];
        }
    }
    const int half = shift > 0 ? 1 << (shift - 1) : 0;
    uint8_t* dp = dst + ((long long)s * npx + pix) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) dp[c] = (uint8_t)((acc[c] + half) >> shift);
}

// ---- median blur -----------------------------------------------------------------------------------------------------------------------------------
// The median of K x K values by rank counting: v is the median iff #(values < v) <= M < #(values <= v), M = K K / 2.  No data-dependent indexing:
// the window stays in registers (three channels packed into one word per tap).
template <int K>
__device__ __forceinline__ void aug_median_px(const uint8_t* __restrict__ sp, int h, int w, int y, int x, uint8_t out[3]) {
    constexpr int R = K / 2, N = K * K, M = N / 2;
    uint32_t tap[N];
#pragma unroll
    for (int dy = 0; dy < K; ++dy) {
        const int yy = min(max(y + dy - R, 0), h - 1);
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
            const int xx = min(max(x + dx - R, 0), w - 1);
            const uint8_t* q = sp + ((long long)yy * w + xx) * 3;
            tap[dy * K + dx] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int med = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int vi = (int)((tap[i] >> (8 * c)) & 255u);
            int lt = 0, le = 0;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int vj = (int)((tap[j] >> (8 * c)) & 255u);
                lt += vj < vi, le += vj <= vi;
            }
            if (lt <= M && M < le) med = vi;
        }
        out[c] = (uint8_t)med;
    }
}

__global__ __launch_bounds__(AUG_BLOCK) void aug_median_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int w,
                                                               const int32_t* __restrict__ ks) {
    const int s = blockIdx.y;
    const int k = ks[s];
    if (!aug_ksize_ok(k)) return;  // 0 (or anything else): the sample is not written
    const long long npx = (long long)h * w, pix = (long long)blockIdx.x * AUG_BLOCK + threadIdx.x;
    if (pix >= npx) return;
    const int y = (int)(pix / w), x = (int)(pix - (long long)y * w);
    const uint8_t* sp = src + (long long)s * npx * 3;
    uint8_t o[3];
    if (k == 5)
        aug_median_px<5>(sp, h, w, y, x, o);
    else if (k == 3)
        aug_median_px<3>(sp, h, w, y, x, o);
    else
        aug_median_px<1>(sp, h, w, y, x, o);
    uint8_t* dp = dst + ((long long)s * npx + pix) * 3;
    dp[0] = o[0], dp[1] = o[1], dp[2] = o[2];
}

// ---- Gaussian noise --------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void aug_philox(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t r[4]) {  // Philox4x32-10, counter (c0, c1, 0, 0)
    uint32_t c2 = 0, c3 = 0;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

__global__ __launch_bounds__(AUG_BLOCK) void aug_noise_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long npx, bool vec,
                                                              const double* __restrict__ sigma, const int32_t* __restrict__ per_channel,
                                                              const u64* __restrict__ keys) {
    const int s = blockIdx.y;
    const double sg = sigma[s];
    if (!aug_finite(sg)) return;  // NaN: the sample is not written
    const bool pc = per_channel[s] != 0;
    const u64 key = keys[s];
    const long long g = (long long)blockIdx.x * AUG_BLOCK + threadIdx.x;
    uint8_t b[12];
    const int cnt = aug_load4(src + (long long)s * npx * 3, g, npx, vec, b);
    if (cnt == 0) return;
    constexpr double TWO_PI = 6.283185307179586, INV32 = 1.0 / 4294967296.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const u64 pix = (u64)(g * 4 + i);
        uint32_t r[4];
        aug_philox((uint32_t)pix, (uint32_t)(pix >> 32), (uint32_t)key, (uint32_t)(key >> 32), r);
        const double u1 = ((double)r[0] + 1.0) * INV32, u2 = (double)r[1] * INV32;
        const double rad = sqrt(-2.0 * log(u1)), ang = TWO_PI * u2;
        double z[3];
        z[0] = rad * cos(ang);
        if (pc) {
            const double u3 = ((double)r[2] + 1.0) * INV32, u4 = (double)r[3] * INV32;
            z[1] = rad * sin(ang);
            z[2] = sqrt(-2.0 * log(u3)) * cos(TWO_PI * u4);
        } else {
            z[1] = z[2] = z[0];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double x = floor((double)b[i * 3 + c] + sg * z[c] + 0.5);
            b[i * 3 + c] = aug_clip_trunc(x);
        }
    }
    aug_store4(dst + (long long)s * npx * 3, g, cnt, vec, b);
}

// ---- colour ----------------------------------------------------------------------------------------------------------------------------------------
// op: 0 brightness, 1 saturation, 2 hue, 3 contrast.  A sample whose value is not finite is skipped: copied when dst != src, left alone in place.
__device__ __forceinline__ void aug_hue_px(uint8_t* px, double hue) {
    const int R = px[0], G = px[1], B = px[2];
    const int V = max(R, max(G, B)), mn = min(R, min(G, B)), d = V - mn;
    const int S = V == 0 ? 0 : (510 * d + V) / (2 * V);
    int H = 0;
    if (d != 0) {
        const int hnum = V == R ? G - B : (V == G ? (B - R) + 2 * d : (R - G) + 4 * d);
        const int num = 60 * hnum + d, den = 2 * d;
        H = num >= 0 ? num / den : -((-num + den - 1) / den);  // floor
        if (H < 0) H += 180;
        if (H >= 180) H -= 180;
    }
    double r = fmod((double)H + hue, 180.0);
    if (r < 0.0) r += 180.0;  // the divisor's sign (may round to 180.0 itself: sector 6 below is sector 0)
    const double Hs = trunc(r);
    const double s = (double)S / 255.0, v = (double)V, hh = Hs / 30.0, fl = floor(hh), f = hh - fl;
    const int sector = (int)fl % 6;
    const double p = v * (1.0 - s), q = v * (1.0 - s * f), t = v * (1.0 - s * (1.0 - f));
    double o0, o1, o2;
    switch (sector) {
        case 0: o0 = v, o1 = t, o2 = p; break;
        case 1: o0 = q, o1 = v, o2 = p; break;
        case 2: o0 = p, o1 = v, o2 = t; break;
        case 3: o0 = p, o1 = q, o2 = v; break;
        case 4: o0 = t, o1 = p, o2 = v; break;
        default: o0 = v, o1 = p, o2 = q; break;
    }
    px[0] = aug_clip_trunc(rint(o0)), px[1] = aug_clip_trunc(rint(o1)), px[2] = aug_clip_trunc(rint(o2));
}

template <int OP>
__global__ __launch_bounds__(AUG_BLOCK) void aug_colour_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long npx, bool vec,
                                                               const double* __restrict__ value, const long long* __restrict__ sums) {
    const int s = blockIdx.y;
    const double val = value[s];
    const bool skip = !aug_finite(val);
    if (skip && src == dst) return;
    const long long g = (long long)blockIdx.x * AUG_BLOCK + threadIdx.x;
    uint8_t b[12];
    const int cnt = aug_load4(src + (long long)s * npx * 3, g, npx, vec, b);
    if (cnt == 0) return;
    if (!skip) {
        double mean[3] = {0.0, 0.0, 0.0};
        if (OP == 3) {
#pragma unroll
            for (int c = 0; c < 3; ++c) mean[c] = (double)sums[(long long)s * 3 + c] / (double)npx;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint8_t* px = b + i * 3;
            if (OP == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) px[c] = aug_clip_trunc((double)px[c] + val);
            } else if (OP == 1) {
                const double gray = (double)((4899 * px[0] + 9617 * px[1] + 1868 * px[2] + 8192) >> 14), sc = 1.0 + val, rest = gray * (1.0 - sc);
#pragma unroll
                for (int c = 0; c < 3; ++c) px[c] = aug_clip_trunc((double)px[c] * sc + rest);
            } else if (OP == 2) {
                aug_hue_px(px, val);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) px[c] = aug_clip_trunc((double)px[c] * val + mean[c] * (1.0 - val));
            }
        }
    }
    aug_store4(dst + (long long)s * npx * 3, g, cnt, vec, b);
}

// ---- channel sums ----------------------------------------------------------------------------------------------------------------------------------
// Integer partial sums per thread and per wave, one 64-bit integer atomic per (wave, channel): exact in any arrival order.
__global__ __launch_bounds__(AUG_BLOCK) void aug_sums_kernel(const uint8_t* __restrict__ src, long long npx, bool vec, u64* __restrict__ sums) {
    const int s = blockIdx.y;
    const uint8_t* sp = src + (long long)s * npx * 3;
    unsigned acc[3] = {0, 0, 0};
#pragma unroll 1
    for (int it = 0; it < AUG_SUM_ITERS; ++it) {
        const long long g = ((long long)blockIdx.x * AUG_SUM_ITERS + it) * AUG_BLOCK + threadIdx.x;
        const long long first = g * 4;
        if (first >= npx) break;
        if (vec && npx - first >= 4) {  // bytes R G B R | G B R G | B R G B
            const uint32_t* q = reinterpret_cast<const uint32_t*>(sp + first * 3);
            const uint32_t a0 = q[0], a1 = q[1], a2 = q[2];
            acc[0] += (a0 & 255u) + (a0 >> 24) + ((a1 >> 16) & 255u) + ((a2 >> 8) & 255u);
            acc[1] += ((a0 >> 8) & 255u) + (a1 & 255u) + (a1 >> 24) + ((a2 >> 16) & 255u);
            acc[2] += ((a0 >> 16) & 255u) + ((a1 >> 8) & 255u) + (a2 & 255u) + (a2 >> 24);
        } else {
            const long long last = npx - first < 4 ? npx : first + 4;
            for (long long px = first; px < last; ++px) acc[0] += sp[px * 3], acc[1] += sp[px * 3 + 1], acc[2] += sp[px * 3 + 2];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        unsigned v = acc[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(sums + (long long)s * 3 + c, (u64)v);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------------
int aug_shape(const char* who, int n, int h, int w) {
    if (n < 1 || n > AUG_MAX_N) return fail(std::string(who) + ": batch size outside 1 .. 65535");
    if (h < 1 || w < 1) return fail(std::string(who) + ": empty image");
    if (h > AUG_MAX_SIDE || w > AUG_MAX_SIDE) return fail(std::string(who) + ": side above 16384");
    return 0;
}
bool aug_overlap(const void* a, long long a_bytes, const void* b, long long b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)b_bytes && y < x + (uintptr_t)a_bytes;
}
inline dim3 aug_grid(long long items, int n) { return dim3((unsigned)((items + AUG_BLOCK - 1) / AUG_BLOCK), (unsigned)n); }
// three-dword access of a pixel group needs every sample's first byte 4-byte aligned
inline bool aug_vec_ok(const void* a, const void* b, long long npx) { return (uintptr_t)a % 4 == 0 && (uintptr_t)b % 4 == 0 && (npx * 3) % 4 == 0; }

template <int OP>
int aug_colour(const char* who, const uint8_t* src, uint8_t* dst, int n, int h, int w, const double* value, const long long* sums, void* hip_stream) {
    if (src == nullptr || dst == nullptr || value == nullptr || (OP == 3 && sums == nullptr)) return fail(std::string(who) + ": null pointer");
    if (aug_shape(who, n, h, w)) return 1;
    const long long npx = (long long)h * w, bytes = npx * 3 * n;
    if (src != dst && aug_overlap(src, bytes, dst, bytes)) return fail(std::string(who) + ": src and dst overlap without being equal");
    hipLaunchKernelGGL(aug_colour_kernel<OP>, aug_grid((npx + 3) / 4, n), dim3(AUG_BLOCK), 0, (hipStream_t)hip_stream, src, dst, npx,
                       aug_vec_ok(src, dst, npx), value, sums);
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int cerb_aug_warp(const uint8_t* img, const int32_t* ann, int n, int src_h, int src_w, int ann_c, const int64_t* maps, uint8_t* img_out,
                             int32_t* ann_out, int out_h, int out_w, void* hip_stream) {
    if (maps == nullptr || (img == nullptr && ann == nullptr)) return fail("cerb_aug_warp: null pointer");
    if ((img == nullptr) != (img_out == nullptr) || (ann == nullptr) != (ann_out == nullptr)) return fail("cerb_aug_warp: an input without its output (or the reverse)");
    if (aug_shape("cerb_aug_warp", n, src_h, src_w) || aug_shape("cerb_aug_warp", n, out_h, out_w)) return 1;
    if (ann != nullptr && (ann_c < 1 || ann_c > 8)) return fail("cerb_aug_warp: annotation channels outside 1 .. 8");
    const long long spx = (long long)n * src_h * src_w, dpx = (long long)n * out_h * out_w;
    if (img != nullptr && aug_overlap(img, spx * 3, img_out, dpx * 3)) return fail("cerb_aug_warp: img and img_out overlap (the gather is out of place)");
    if (ann != nullptr && aug_overlap(ann, spx * ann_c * 4, ann_out, dpx * ann_c * 4)) return fail("cerb_aug_warp: ann and ann_out overlap (the gather is out of place)");
    hipLaunchKernelGGL(aug_warp_kernel, aug_grid((long long)out_h * out_w, n), dim3(AUG_BLOCK), 0, (hipStream_t)hip_stream, img, ann, src_h, src_w, ann_c,
                       (const long long*)maps, img_out, ann_out, out_h, out_w);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int cerb_aug_gaussian_blur(const uint8_t* src, uint8_t* dst, int n, int h, int w, const int32_t* kx, const int32_t* ky, void* hip_stream) {
    if (src == nullptr || dst == nullptr || kx == nullptr || ky == nullptr) return fail("cerb_aug_gaussian_blur: null pointer");
    if (aug_shape("cerb_aug_gaussian_blur", n, h, w)) return 1;
    const long long bytes = (long long)n * h * w * 3;
    if (aug_overlap(src, bytes, dst, bytes)) return fail("cerb_aug_gaussian_blur: src and dst overlap (the stencil is out of place)");
    hipLaunchKernelGGL(aug_gauss_kernel, aug_grid((long long)h * w, n), dim3(AUG_BLOCK), 0, (hipStream_t)hip_stream, src, dst, h, w, kx, ky);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int cerb_aug_median_blur(const uint8_t* src, uint8_t* dst, int n, int h, int w, const int32_t* k, void* hip_stream) {
    if (src == nullptr || dst == nullptr || k == nullptr) return fail("cerb_aug_median_blur: null pointer");
    if (aug_shape("cerb_aug_median_blur", n, h, w)) return 1;
    const long long bytes = (long long)n * h * w * 3;
    if (aug_overlap(src, bytes, dst, bytes)) return fail("cerb_aug_median_blur: src and dst overlap (the stencil is out of place)");
    hipLaunchKernelGGL(aug_median_kernel, aug_grid((long long)h * w, n), dim3(AUG_BLOCK), 0, (hipStream_t)hip_stream, src, dst, h, w, k);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int cerb_aug_gaussian_noise(const uint8_t* src, uint8_t* dst, int n, int h, int w, const double* sigma, const int32_t* per_channel,
                                       const uint64_t* key, void* hip_stream) {
    if (src == nullptr || dst == nullptr || sigma == nullptr || per_channel == nullptr || key == nullptr) return fail("cerb_aug_gaussian_noise: null pointer");
    if (aug_shape("cerb_aug_gaussian_noise", n, h, w)) return 1;
    const long long npx = (long long)h * w, bytes = npx * 3 * n;
    if (src != dst && aug_overlap(src, bytes, dst, bytes)) return fail("cerb_aug_gaussian_noise: src and dst overlap without being equal");
    hipLaunchKernelGGL(aug_noise_kernel, aug_grid((npx + 3) / 4, n), dim3(AUG_BLOCK), 0, (hipStream_t)hip_stream, src, dst, npx, aug_vec_ok(src, dst, npx), sigma,
                       per_channel, (const u64*)key);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int cerb_aug_brightness(const uint8_t* src, uint8_t* dst, int n, int h, int w, const double* value, void* hip_stream) {
    return aug_colour<0>("cerb_aug_brightness", src, dst, n, h, w, value, nullptr, hip_stream);
}
extern "C" int cerb_aug_saturation(const uint8_t* src, uint8_t* dst, int n, int h, int w, const double* value, void* hip_stream) {
    return aug_colour<1>("cerb_aug_saturation", src, dst, n, h, w, value, nullptr, hip_stream);
}
extern "C" int cerb_aug_hue(const uint8_t* src, uint8_t* dst, int n, int h, int w, const double* value, void* hip_stream) {
    return aug_colour<2>("cerb_aug_hue", src, dst, n, h, w, value, nullptr, hip_stream);
}
extern "C" int cerb_aug_contrast(const uint8_t* src, uint8_t* dst, int n, int h, int w, const double* value, const int64_t* sums, void* hip_stream) {
    return aug_colour<3>("cerb_aug_contrast", src, dst, n, h, w, value, (const long long*)sums, hip_stream);
}

extern "C" int cerb_aug_channel_sums(const uint8_t* src, int n, int h, int w, int64_t* sums, void* hip_stream) {
    if (src == nullptr || sums == nullptr) return fail("cerb_aug_channel_sums: null pointer");
    if (aug_shape("cerb_aug_channel_sums", n, h, w)) return 1;
    const long long npx = (long long)h * w;
    HIP_OK(hipMemsetAsync(sums, 0, (size_t)n * 3 * sizeof(int64_t), (hipStream_t)hip_stream));
    const long long per_block = (long long)AUG_BLOCK * AUG_SUM_ITERS, groups = (npx + 3) / 4;
    hipLaunchKernelGGL(aug_sums_kernel, dim3((unsigned)((groups + per_block - 1) / per_block), (unsigned)n), dim3(AUG_BLOCK), 0, (hipStream_t)hip_stream, src, npx,
                       aug_vec_ok(src, src, npx), (u64*)sums);
    HIP_OK(hipGetLastError());
    return 0;
}
