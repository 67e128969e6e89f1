// JPEG tiles of a TIFF / .svs level, decoded for the slide driver without the interpreter (include/cerberus_hip.h, "JPEG tiles"):
//   cerb_jpeg_read_tiles    : HOST.  pread + marker parse + Huffman pass (jpeg_entropy.h) of a window's tiles on pthreads that take tiles off a shared
//                             counter (the scheme of cerb_host_tiff_read_tiles) -> per-tile headers + quantised int16 coefficients in the caller's
//                             (pinned) buffer.  The only serial part of a baseline JPEG decode.
//   cerb_jpeg_decode_window : DEVICE, two launches on the caller's stream.
//                             jpeg_idct_kernel  -- dequantise + 8 x 8 inverse DCT ("islow": 13-bit constants, columns then rows) into per-tile component
//                                                  planes (uint8) in a caller-provided scratch; one block per 8 lanes, 8 blocks per wave;
//                             jpeg_place_kernel -- chroma up-sampling (libjpeg's "fancy" triangle filters), YCbCr -> RGB, and the part of every tile
//                                                  inside the window written to dst.
// Every product is defined in 64-bit integers (a dequantised coefficient of a stream the entropy decoder accepts can be 2^31, pass 1 then reaches 2^37);
// both passes are bound by memory, not by these multiplies.  Equal to PIL / libjpeg-turbo bit for bit on every stream an encoder writes
// (tests/test_jpeg_host.py states the same arithmetic in numpy, tests/test_jpeg_gpu.py runs it here).
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <unistd.h>

#include <atomic>
#include <cstddef>
#include <string>

#include "../../include/cerberus_hip.h"
#include "jpeg_entropy.h"

int cerb_set_error(const std::string& m);

static_assert(sizeof(cerb_jpeg_hdr) == 464 && offsetof(cerb_jpeg_hdr, q) == 80, "cerb_jpeg_hdr layout (cerberus_amd/jpeg_device.py mirrors it)");

// ---- buffer layout -----------------------------------------------------------------------------------------------------------------------------
// stream buffer (pinned on the host, one copy to the device): n_tiles headers, padded to 256 bytes, then the coefficients of the tiles that decoded,
// packed in the order their threads claimed room.  A tile never needs more than 3 samples per pixel of its 16-aligned size (4:4:4).
static inline long long jpeg_tile_cap(int tile_w, int tile_h) { return 3LL * ((tile_w + 15) / 16 * 16) * ((tile_h + 15) / 16 * 16); }
static inline size_t jpeg_coef_base(int n_tiles) { return ((size_t)n_tiles * sizeof(cerb_jpeg_hdr) + 255) / 256 * 256; }

extern "C" size_t cerb_jpeg_workspace_bytes(int n_tiles, int tile_w, int tile_h, int which) {
    if (n_tiles < 0 || tile_w < 1 || tile_h < 1 || tile_w > 65535 || tile_h > 65535) return 0;
    const size_t samples = (size_t)n_tiles * (size_t)jpeg_tile_cap(tile_w, tile_h);
    return which == 0 ? jpeg_coef_base(n_tiles) + samples * sizeof(int16_t) : samples;
}

extern "C" int cerb_jpeg_decode_stream(const uint8_t* tables, long long n_tables, const uint8_t* src, long long n_src, int photometric_rgb, void* hdr,
                                       int16_t* coefs, long long coef_cap, long long* coef_used) {
    cerb_jpeg_hdr local;
    int64_t used = 0;
    const int rc = (!src || n_src < 0 || !coefs || coef_cap < 0) ? CERB_JPEG_CORRUPT
                                                                  : cerb_jpeg_entropy_decode(tables, n_tables, src, n_src, photometric_rgb, &local, coefs, coef_cap, &used);
    if (hdr) memcpy(hdr, &local, sizeof(local));
    if (coef_used) *coef_used = used;
    return rc;
}

// ---- host half -----------------------------------------------------------------------------------------------------------------------------------
struct jpeg_job {
    int fd, n_tiles, tile_w, tile_h, photometric_rgb;
    const int64_t *offsets, *counts;
    const int32_t *gx0, *gy0;
    const uint8_t* tables;
    int64_t n_tables;
    cerb_jpeg_hdr* hdrs;
    int16_t* coefs;
    long long coef_cap;
    std::atomic<int> next{0};
    std::atomic<long long> cursor{0};
    std::atomic<int> err{0};       // 0 fine, -1 a corrupt tile, -3 short read, -6 no memory
    std::atomic<int> bad_tile{-1}; // the lowest index among the tiles that failed
};

static int64_t jpeg_pread_all(int fd, uint8_t* buf, int64_t n, int64_t off) {
    int64_t got = 0;
    while (got < n) {
        const ssize_t r = pread(fd, buf + got, (size_t)(n - got), (off_t)(off + got));
        if (r <= 0) break;
        got += r;
    }
    return got;
}

static void* jpeg_worker(void* arg) {
    jpeg_job* j = (jpeg_job*)arg;
    uint8_t* raw = nullptr;
    int64_t raw_cap = 0;
    cerb_jpeg_state* st = (cerb_jpeg_state*)malloc(sizeof(cerb_jpeg_state));
    for (;;) {
        const int i = j->next.fetch_add(1);
        if (i >= j->n_tiles || j->err.load()) break;
        cerb_jpeg_hdr* hdr = &j->hdrs[i];
        memset(hdr, 0, sizeof(*hdr));
        int kind = 0;
        const int64_t cnt = j->counts[i];
        if (cnt > raw_cap) {
            free(raw);
            raw = (uint8_t*)malloc((size_t)cnt + 8);
            raw_cap = raw ? cnt : 0;
        }
        if (!st || cnt < 0 || (cnt > 0 && !raw)) {
            kind = -6;
        } else if (jpeg_pread_all(j->fd, raw, cnt, j->offsets[i]) != cnt) {
            kind = -3;
        } else {
            int64_t scan_pos = 0;
            int rc = cerb_jpeg_parse_tile(st, j->tables, j->n_tables, raw, cnt, &scan_pos);
            if (rc == CERB_JPEG_OK) {
                const int64_t need = cerb_jpeg_fill_hdr(st, j->photometric_rgb, hdr);
                // a stream of another size than the level's tiles goes the caller's other way (it crops or refuses it as it always has)
                if (hdr->width != j->tile_w || hdr->height != j->tile_h) {
                    rc = CERB_JPEG_UNSUPPORTED;
                } else {
                    const long long off = j->cursor.fetch_add(need);
                    if (off + need > j->coef_cap) rc = CERB_JPEG_TOO_LARGE;  // (cannot happen in a buffer of cerb_jpeg_workspace_bytes)
                    else {
                        hdr->coef_off = off;
                        rc = cerb_jpeg_scan(st, hdr, raw, cnt, scan_pos, j->coefs + off);
                    }
                }
            }
            hdr->status = rc;
            hdr->gx0 = j->gx0[i];
            hdr->gy0 = j->gy0[i];
            if (rc < 0) kind = -1;
        }
        if (kind) {
            hdr->status = CERB_JPEG_CORRUPT;
            int zero = 0;
            j->err.compare_exchange_strong(zero, kind);
            int cur = j->bad_tile.load();
            while ((cur < 0 || i < cur) && !j->bad_tile.compare_exchange_weak(cur, i)) {
            }
            break;
        }
    }
    free(raw);
    free(st);
    return nullptr;
}

extern "C" int cerb_jpeg_read_tiles(int fd, int n_tiles, const int64_t* offsets, const int64_t* counts, const int32_t* gx0, const int32_t* gy0, int tile_w,
                                    int tile_h, const uint8_t* tables, long long n_tables, int photometric_rgb, void* buf, size_t buf_bytes, int n_threads,
                                    size_t* used_bytes, int32_t* bad_tile, int32_t* n_unsupported, int32_t* unsupported) {
    if (bad_tile) *bad_tile = -1;
    if (n_unsupported) *n_unsupported = 0;
    if (used_bytes) *used_bytes = 0;
    if (n_tiles < 0 || (n_tiles > 0 && (!offsets || !counts || !gx0 || !gy0)) || tile_w < 1 || tile_h < 1 || tile_w > 65535 || tile_h > 65535 || !buf ||
        !used_bytes || !bad_tile || !n_unsupported || !unsupported || (n_tables > 0 && !tables) || ((uintptr_t)buf & 15))
        return cerb_set_error("cerb_jpeg_read_tiles: bad arguments");
    const size_t base = jpeg_coef_base(n_tiles);
    if (buf_bytes < base) return cerb_set_error("cerb_jpeg_read_tiles: the buffer does not hold the tile headers");
    jpeg_job j;
    j.fd = fd; j.n_tiles = n_tiles; j.tile_w = tile_w; j.tile_h = tile_h; j.photometric_rgb = photometric_rgb;
    j.offsets = offsets; j.counts = counts; j.gx0 = gx0; j.gy0 = gy0; j.tables = n_tables > 0 ? tables : nullptr; j.n_tables = n_tables > 0 ? n_tables : 0;
    j.hdrs = (cerb_jpeg_hdr*)buf;
    j.coefs = (int16_t*)((uint8_t*)buf + base);
    j.coef_cap = (long long)((buf_bytes - base) / sizeof(int16_t));
    if (n_threads > n_tiles) n_threads = n_tiles;
    if (n_threads > 64) n_threads = 64;
    pthread_t th[64];
    int started = 0;
    for (int t = 1; t < n_threads; ++t) {
        if (pthread_create(&th[started], nullptr, jpeg_worker, &j) != 0) break;  // fewer threads than asked for: the others take the tiles
        ++started;
    }
    jpeg_worker(&j);
    for (int t = 0; t < started; ++t) pthread_join(th[t], nullptr);
    const long long used = j.cursor.load() < j.coef_cap ? j.cursor.load() : j.coef_cap;
    *used_bytes = base + (size_t)used * sizeof(int16_t);
    *bad_tile = j.bad_tile.load();
    const int err = j.err.load();
    if (err == -1) return cerb_set_error("cerb_jpeg_read_tiles: tile " + std::to_string(*bad_tile) + " of the call is not a decodable JPEG stream (truncated or corrupt)");
    if (err == -3) return cerb_set_error("cerb_jpeg_read_tiles: short read of tile " + std::to_string(*bad_tile));
    if (err) return cerb_set_error("cerb_jpeg_read_tiles: out of host memory");
    int nu = 0;
    for (int i = 0; i < n_tiles; ++i)
        if (j.hdrs[i].status == CERB_JPEG_UNSUPPORTED) unsupported[nu++] = i;
    *n_unsupported = nu;
    return 0;
}

// ---- device half ---------------------------------------------------------------------------------------------------------------------------------
// One 1-D pass of the "islow" inverse DCT (CONST_BITS 13); the caller shifts.
__device__ __forceinline__ void jpeg_idct_1d(const long long i[8], long long o[8]) {
    long long z1 = (i[2] + i[6]) * 4433;
    const long long t2 = z1 - i[6] * 15137, t3 = z1 + i[2] * 6270;
    const long long t0 = (i[0] + i[4]) * 8192, t1 = (i[0] - i[4]) * 8192;
    const long long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    long long u0 = i[7], u1 = i[5], u2 = i[3], u3 = i[1];
    z1 = u0 + u3;
    long long z2 = u1 + u2, z3 = u0 + u2, z4 = u1 + u3;
    const long long z5 = (z3 + z4) * 9633;
    u0 *= 2446; u1 *= 16819; u2 *= 25172; u3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    u0 += z1 + z3; u1 += z2 + z4; u2 += z2 + z3; u3 += z1 + z4;
    o[0] = t10 + u3; o[7] = t10 - u3;
    o[1] = t11 + u2; o[6] = t11 - u2;
    o[2] = t12 + u1; o[5] = t12 - u1;
    o[3] = t13 + u0; o[4] = t13 - u0;
}

// grid (ceil(blocks of the largest tile / 32), n_tiles), 256 threads: 8 lanes own one 8 x 8 block.  Lane l loads coefficient row l as one 16-byte
// vector, the block is transposed through LDS so that the lane runs pass 1 down column l, transposed back (64-bit words: pass 1 leaves up to 2^37),
// pass 2 runs along row l and the lane stores its 8 samples as one 8-byte vector.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const cerb_jpeg_hdr* __restrict__ hdrs, const int16_t* __restrict__ coefs, long long coef_total,
                                                        uint8_t* __restrict__ planes) {
    __shared__ int ws1[32][8][9];
    __shared__ long long ws2[32][8][9];
    const cerb_jpeg_hdr* hd = hdrs + blockIdx.y;
    const int l = threadIdx.x & 7, g = threadIdx.x >> 3;
    const long long blk = (long long)blockIdx.x * 32 + g;
    const int mcus = hd->mcu_cols * hd->mcu_rows;
    const long long nb0 = (long long)mcus * hd->h[0] * hd->v[0], total = nb0 + 2LL * mcus;
    const long long off = hd->coef_off;
    const bool valid = hd->status == 0 && blk < total && off >= 0 && off + total * 64 <= coef_total;
    int comp = 0;
    long long li = blk, across = (long long)hd->mcu_cols * hd->h[0];
    if (blk >= nb0) {
        comp = blk < nb0 + mcus ? 1 : 2;
        li = blk - nb0 - (comp == 2 ? mcus : 0);
        across = hd->mcu_cols;
    }
    if (valid) {
        const int4 raw = *reinterpret_cast<const int4*>(coefs + off + blk * 64 + l * 8);
        const uint4 qv = *reinterpret_cast<const uint4*>(&hd->q[comp][l * 8]);
        const int c[4] = {raw.x, raw.y, raw.z, raw.w};
        const unsigned q[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ws1[g][l][2 * k] = (int)(short)(c[k] & 0xFFFF) * (int)(q[k] & 0xFFFF);       // |c q| <= 32768 * 65535 < 2^31
            ws1[g][l][2 * k + 1] = (c[k] >> 16) * (int)(q[k] >> 16);
        }
    }
    __syncthreads();
    long long in[8], out[8];
    if (valid) {
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = ws1[g][r][l];
        jpeg_idct_1d(in, out);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws2[g][r][l] = (out[r] + 1024) >> 11;
    }
    __syncthreads();
    if (valid) {
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = ws2[g][l][k];
        jpeg_idct_1d(in, out);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            long long s = ((out[k] + 131072) >> 18) + 128;
            s = s < 0 ? 0 : (s > 255 ? 255 : s);
            if (k < 4) lo |= (unsigned)s << (8 * k);
            else hi |= (unsigned)s << (8 * (k - 4));
        }
        const long long br = li / across, bc = li - br * across;
        uint8_t* p = planes + off + (blk - li) * 64 + (br * 8 + l) * (across * 8) + bc * 8;
        *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi);
    }
}

struct jpeg_planes {
    const uint8_t *y, *cb, *cr;
    int ys, cs;      // row strides
    int cw, ch;      // the chroma planes' true size: the up-sampling filters replicate at THESE edges, not at the padded block grid's
    int mode;        // 0: 4:4:4, 1: 4:2:2 (h2v1), 2: 4:2:0 (h2v2)
    int transform;
};

__device__ __forceinline__ int jpeg_chroma(const uint8_t* pl, const jpeg_planes& P, int tx, int ty) {
    if (P.mode == 0) return pl[(long long)ty * P.cs + tx];
    const int i = tx >> 1;
    if (P.mode == 1) {
        const uint8_t* row = pl + (long long)ty * P.cs;
        if (tx == 0 || tx == 2 * P.cw - 1) return row[i];
        return (tx & 1) ? (3 * row[i] + row[i + 1] + 2) >> 2 : (3 * row[i] + row[i - 1] + 1) >> 2;
    }
    const int r = ty >> 1;
    int r2 = (ty & 1) ? r + 1 : r - 1;
    r2 = r2 < 0 ? 0 : (r2 > P.ch - 1 ? P.ch - 1 : r2);
    const uint8_t *a = pl + (long long)r * P.cs, *b = pl + (long long)r2 * P.cs;
    const int s = 3 * a[i] + b[i];
    if (tx & 1) {
        const int i2 = i + 1 > P.cw - 1 ? P.cw - 1 : i + 1;
        return (3 * s + 3 * a[i2] + b[i2] + 7) >> 4;
    }
    const int i2 = i - 1 < 0 ? 0 : i - 1;
    return (3 * s + 3 * a[i2] + b[i2] + 8) >> 4;
}

__device__ __forceinline__ unsigned jpeg_pixel(const jpeg_planes& P, int tx, int ty) {
    const int y = P.y[(long long)ty * P.ys + tx];
    int c1 = jpeg_chroma(P.cb, P, tx, ty), c2 = jpeg_chroma(P.cr, P, tx, ty);
    int r = y, g = c1, b = c2;
    if (P.transform) {
        c1 -= 128;
        c2 -= 128;
        r = y + ((91881 * c2 + 32768) >> 16);
        g = y + ((-22554 * c1 - 46802 * c2 + 32768) >> 16);
        b = y + ((116130 * c1 + 32768) >> 16);
        r = r < 0 ? 0 : (r > 255 ? 255 : r);
        g = g < 0 ? 0 : (g > 255 ? 255 : g);
        b = b < 0 ? 0 : (b > 255 ? 255 : b);
    }
    return (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16);
}

// grid (ceil(rows x quads of a tile / 256), n_tiles).  A thread owns 4 consecutive pixels of one window row, on a 4-pixel grid of the WINDOW's columns:
// their 12 bytes start on a 4-byte boundary of an aligned destination and leave as one 12-byte store; quads cut by the tile's or the window's edge, and
// unaligned destinations, store bytes.
__global__ __launch_bounds__(256) void jpeg_place_kernel(const cerb_jpeg_hdr* __restrict__ hdrs, const uint8_t* __restrict__ planes, long long plane_total,
                                                         uint8_t* __restrict__ dst, long long dst_row_stride, int x0, int y0, int x1, int y1, int aligned) {
    const cerb_jpeg_hdr* hd = hdrs + blockIdx.y;
    if (hd->status != 0) return;
    const int W = hd->width, H = hd->height, gx0 = hd->gx0, gy0 = hd->gy0;
    const int a0 = max(y0, gy0), a1 = min(y1, gy0 + H), b0 = max(x0, gx0), b1 = min(x1, gx0 + W);
    if (a1 <= a0 || b1 <= b0) return;
    const int mcus = hd->mcu_cols * hd->mcu_rows, h0 = hd->h[0], v0 = hd->v[0];
    const long long nb0 = (long long)mcus * h0 * v0, off = hd->coef_off;
    if (off < 0 || off + (nb0 + 2LL * mcus) * 64 > plane_total) return;
    jpeg_planes P;
    P.y = planes + off;
    P.cb = P.y + nb0 * 64;
    P.cr = P.cb + (long long)mcus * 64;
    P.ys = hd->mcu_cols * h0 * 8;
    P.cs = hd->mcu_cols * 8;
    P.cw = (W + h0 - 1) / h0;
    P.ch = (H + v0 - 1) / v0;
    P.mode = h0 == 1 ? 0 : (v0 == 1 ? 1 : 2);
    P.transform = hd->transform;
    const int c0 = b0 - x0, c1 = b1 - x0, q0 = c0 >> 2, nq = ((c1 + 3) >> 2) - q0;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)nq * (a1 - a0)) return;
    const int r = (int)(idx / nq), q = q0 + (int)(idx - (long long)r * nq);
    const int y = a0 + r, ty = y - gy0;
    uint8_t* row = dst + (long long)(y - y0) * dst_row_stride;
    const int col = q * 4;
    if (aligned && col >= c0 && col + 4 <= c1) {
        const int tx = col + x0 - gx0;
        const unsigned p0 = jpeg_pixel(P, tx, ty), p1 = jpeg_pixel(P, tx + 1, ty), p2 = jpeg_pixel(P, tx + 2, ty), p3 = jpeg_pixel(P, tx + 3, ty);
        struct alignas(4) u3 { unsigned a, b, c; };
        *reinterpret_cast<u3*>(row + (long long)col * 3) = u3{p0 | (p1 << 24), (p1 >> 8) | (p2 << 16), (p2 >> 16) | (p3 << 8)};
        return;
    }
    for (int k = 0; k < 4; ++k) {
        const int c = col + k;
        if (c < c0 || c >= c1) continue;
        const unsigned p = jpeg_pixel(P, c + x0 - gx0, ty);
        row[(long long)c * 3] = (uint8_t)p;
        row[(long long)c * 3 + 1] = (uint8_t)(p >> 8);
        row[(long long)c * 3 + 2] = (uint8_t)(p >> 16);
    }
}

extern "C" int cerb_jpeg_decode_window(const void* dev_buf, size_t dev_bytes, int n_tiles, int tile_w, int tile_h, uint8_t* scratch, size_t scratch_bytes,
                                       uint8_t* dst, long long dst_row_stride, int x0, int y0, int x1, int y1, void* hip_stream) {
    if (!dev_buf || n_tiles < 0 || tile_w < 1 || tile_h < 1 || tile_w > 65535 || tile_h > 65535 || !scratch || !dst || x1 < x0 || y1 < y0 ||
        dst_row_stride < (long long)(x1 - x0) * 3 || ((uintptr_t)dev_buf & 15) || ((uintptr_t)scratch & 7))
        return cerb_set_error("cerb_jpeg_decode_window: bad arguments");
    const size_t base = jpeg_coef_base(n_tiles);
    if (dev_bytes < base) return cerb_set_error("cerb_jpeg_decode_window: the buffer does not hold the tile headers");
    if (n_tiles == 0 || x1 == x0 || y1 == y0) return 0;
    // every offset a header names is checked against what the caller says it copied / reserved: a tile that does not fit is left out, never written past
    long long coef_total = (long long)((dev_bytes - base) / sizeof(int16_t));
    if ((long long)scratch_bytes < coef_total) coef_total = (long long)scratch_bytes;
    const cerb_jpeg_hdr* hdrs = (const cerb_jpeg_hdr*)dev_buf;
    const int16_t* coefs = (const int16_t*)((const uint8_t*)dev_buf + base);
    hipStream_t st = (hipStream_t)hip_stream;
    const long long max_blocks = jpeg_tile_cap(tile_w, tile_h) / 64;
    const long long work = (long long)(tile_w / 4 + 2) * tile_h;
    const int aligned = (((uintptr_t)dst | (uintptr_t)dst_row_stride) & 3) == 0;
    for (int t0 = 0; t0 < n_tiles; t0 += 65535) {  // (the grid's y dimension holds 65535 tiles)
        const int nt = n_tiles - t0 < 65535 ? n_tiles - t0 : 65535;
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + 31) / 32), nt), dim3(256), 0, st, hdrs + t0, coefs, coef_total, scratch);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return cerb_set_error(std::string("kernel launch: ") + hipGetErrorString(e));
        hipLaunchKernelGGL(jpeg_place_kernel, dim3((unsigned)((work + 255) / 256), nt), dim3(256), 0, st, hdrs + t0, (const uint8_t*)scratch, coef_total, dst,
                           dst_row_stride, x0, y0, x1, y1, aligned);
        e = hipGetLastError();
        if (e != hipSuccess) return cerb_set_error(std::string("kernel launch: ") + hipGetErrorString(e));
    }
    return 0;
}
