// Baseline JPEG encoding of a uint8 RGB picture that lives on the device (include/cerberus_hip.h, "JPEG encoding"): the mirror of jpeg_kernels.hip.
//   cerb_jpeg_enc_coefs : jpeg_enc_planes_kernel -- RGB -> Y Cb Cr, edge replication, 4:2:0 down-sampling into padded component planes (workspace);
//                         jpeg_enc_fdct_kernel   -- libjpeg's integer forward DCT ("islow", rows then columns) + quantisation; one block per 8 lanes,
//                                                   8 blocks per wave, transposed through LDS; int16 coefficients in the DECODER's layout.
//   cerb_jpeg_enc_scan  : jpeg_enc_entropy_kernel -- one workgroup per restart interval (= MCU row).  A lane takes a block, forms its symbols twice:
//                                                   once for the bit length, and after a workgroup scan of the lengths once more to deposit the bits
//                                                   (integer atomic OR into the interval's zeroed slot: bit ranges of blocks are disjoint, so the
//                                                   result does not depend on the order);
//                         jpeg_enc_count_kernel  -- FF bytes per interval -> its stuffed length;
//                         jpeg_enc_offsets_kernel -- exclusive scan of the lengths (+ 2 per RSTm marker), the total to a device word;
//                         jpeg_enc_pack_kernel   -- per interval: count / scan / expand (FF -> FF 00) straight into its place of the contiguous scan,
//                                                   the RSTm marker behind it.
//   cerb_jpeg_enc_tiles : the same coefficients cut into tile x tile crops, each an abbreviated stream of its own (prefix, scan, EOI): the entropy and pack
//                         kernels take an interval descriptor (Intervals: MCU rows per stream, MCUs per interval, streams across the picture), so an
//                         interval is one MCU row of ONE TILE -- thousands of workgroups per launch; jpeg_enc_tile_offsets_kernel sums a tile's
//                         intervals, scans the even-padded tile lengths and writes offsets / counts for the caller.
// No call allocates or synchronises; everything is queued on the caller's stream.  Equal to PIL / libjpeg-turbo coefficient for coefficient and, with
// restart_marker_rows = 1, byte for byte in the scan (tests/jpeg_enc_ref.py states the same in numpy).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/cerberus_hip.h"

int cerb_set_error(const std::string& m);

namespace {

// ---- tables (Annex K) ----------------------------------------------------------------------------------------------------------------------------
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t kQLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kQChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
constexpr uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D};
constexpr uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1,
    0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
    0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3,
    0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
constexpr uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1,
    0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A,
    0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA,
    0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};

// (code << 8) | length per symbol, 0 for a symbol the table does not have.  [0] luma, [1] chroma.  Built by the host once per call and passed BY VALUE.
struct HuffTables {
    uint32_t dc[2][12];
    uint32_t ac[2][256];
    uint8_t zigzag[64];
};

void huff_fill(const uint8_t bits[16], const uint8_t* vals, uint32_t* out, int n_out) {
    for (int i = 0; i < n_out; ++i) out[i] = 0;
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {  // Annex C: the codes of one length count up, a longer length doubles the next code
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = (code++ << 8) | (unsigned)len;
        code <<= 1;
    }
}

HuffTables make_huff_tables() {
    HuffTables t;
    huff_fill(kDcLumaBits, kDcVals, t.dc[0], 12);
    huff_fill(kDcChromaBits, kDcVals, t.dc[1], 12);
    huff_fill(kAcLumaBits, kAcLumaVals, t.ac[0], 256);
    huff_fill(kAcChromaBits, kAcChromaVals, t.ac[1], 256);
    for (int i = 0; i < 64; ++i) t.zigzag[i] = kZigzag[i];
    return t;
}

struct QTables {
    uint16_t q[2][64];  // natural order; [0] luma, [1] chroma
};

// ---- geometry ------------------------------------------------------------------------------------------------------------------------------------
struct Geo {
    int w, h, s;         // s: Y's sampling factor both ways (1: 4:4:4, 2: 4:2:0)
    int mr, mc;          // MCU rows / columns
    int yw, yh, cw, ch;  // padded plane sizes
    int bpm;             // blocks per MCU
    long long nb0, nbc;  // blocks of Y, of one chroma component
};

Geo make_geo(int w, int h, int subsampling) {
    Geo g;
    g.w = w; g.h = h; g.s = subsampling == 2 ? 2 : 1;
    g.mr = (h + 8 * g.s - 1) / (8 * g.s);
    g.mc = (w + 8 * g.s - 1) / (8 * g.s);
    g.yw = g.mc * 8 * g.s; g.yh = g.mr * 8 * g.s;
    g.cw = g.mc * 8; g.ch = g.mr * 8;
    g.bpm = g.s * g.s + 2;
    g.nb0 = (long long)g.mr * g.s * g.mc * g.s;
    g.nbc = (long long)g.mr * g.mc;
    return g;
}

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// An interval's room BEFORE stuffing.  With the Annex-K tables a block is at most 11 + 11 bits of DC (longest DC code 11, category <= 11) and
// 63 x (16 + 10) bits of AC (longest AC code 16, category <= 10: 8-bit samples give |AC| <= 1023 at Q = 1): 1660 bits < 208 bytes.  One 32-bit word of
// slack for the last partial word + the pad, rounded to 128 bytes so that intervals never share a cache line.
inline size_t slot_bytes_of(size_t blocks) { return round_up(blocks * 208 + 8, 128); }
inline size_t slot_bytes(const Geo& g) { return slot_bytes_of((size_t)g.mc * g.bpm); }

// workspace of cerb_jpeg_enc_scan: [slots: mr x slot_bytes][raw_len: int32 mr][len: int32 mr][off: int64 mr]
inline size_t scan_ws_bytes(const Geo& g) { return (size_t)g.mr * slot_bytes(g) + round_up((size_t)g.mr * 16, 128); }
// the finished scan at most: every byte of every interval stuffed + the markers
inline size_t scan_cap_bytes(const Geo& g) { return (size_t)g.mr * (2 * ((size_t)g.mc * g.bpm * 208 + 1) + 2); }

// How the MCU grid is cut into restart intervals and the intervals into streams.  Interval iv belongs to stream iv / rows (streams row-major over the
// picture, `across` of them side by side) and is MCU row iv % rows of it: `cols` MCUs.  The whole picture as one stream is {mr, mc, 1}.
struct Intervals {
    int rows, cols, across;
};

// The bytes in front of every tile's scan (SOI SOF0 DRI SOS from the caller), passed BY VALUE.  n = 0 and eoi = 0: the bare scan of cerb_jpeg_enc_scan.
struct StreamEnds {
    int n, eoi;
    uint8_t prefix[64];
};

// tiles: [slots: n_iv x slot][raw_len: int32 n_iv][len: int32 n_iv][off: int64 n_iv], as scan_ws_bytes
inline size_t tiles_ws_bytes(size_t n_iv, size_t slot) { return n_iv * slot + round_up(n_iv * 16, 128); }
// one tile's stream at most: the prefix, every interval stuffed throughout + its marker (RSTm or EOI), the pad byte
inline size_t tile_cap_bytes(const Intervals& it, int bpm) { return round_up(64 + (size_t)it.rows * (2 * ((size_t)it.cols * bpm * 208 + 1) + 2), 2); }

inline size_t planes_bytes(const Geo& g) { return round_up((size_t)g.yw * g.yh + 2 * (size_t)g.cw * g.ch, 128); }

// ---- planes --------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rgb_to_ycc(const uint8_t* p, int& y, int& cb, int& cr) {
    const int r = p[0], g = p[1], b = p[2];
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// One thread per chroma sample: s x s pixels of the padded Y plane.  Columns past the picture replicate the last one at FULL resolution; rows past it
// replicate the last row for Y, and for a down-sampled component ITS last row (ceil(h / 2) - 1), which is libjpeg's order of edge work.
__global__ __launch_bounds__(256) void jpeg_enc_planes_kernel(const uint8_t* __restrict__ src, long long row_stride, Geo g, uint8_t* __restrict__ planes) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)g.cw * g.ch) return;
    const int cy = (int)(idx / g.cw), cx = (int)(idx - (long long)cy * g.cw);
    uint8_t* yp = planes;
    uint8_t* cbp = planes + (long long)g.yw * g.yh;
    uint8_t* crp = cbp + (long long)g.cw * g.ch;
    if (g.s == 1) {
        const int sy = min(cy, g.h - 1), sx = min(cx, g.w - 1);
        int y, cb, cr;
        rgb_to_ycc(src + sy * row_stride + 3LL * sx, y, cb, cr);
        yp[idx] = (uint8_t)y; cbp[idx] = (uint8_t)cb; crp[idx] = (uint8_t)cr;
        return;
    }
    const int chr = (g.h + 1) / 2;           // the chroma component's own rows
    const int ccy = min(cy, chr - 1);        // its last row replicated
    int sb = 0, sr = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int px = min(2 * cx + dx, g.w - 1);
            int y, cb, cr;
            rgb_to_ycc(src + (long long)min(2 * cy + dy, g.h - 1) * row_stride + 3LL * px, y, cb, cr);
            yp[(long long)(2 * cy + dy) * g.yw + 2 * cx + dx] = (uint8_t)y;
            if (ccy != cy) rgb_to_ycc(src + (long long)min(2 * ccy + dy, g.h - 1) * row_stride + 3LL * px, y, cb, cr);
            sb += cb; sr += cr;
        }
    }
    const int bias = 1 + (cx & 1);
    cbp[idx] = (uint8_t)((sb + bias) >> 2);
    crp[idx] = (uint8_t)((sr + bias) >> 2);
}

// ---- forward DCT + quantisation ------------------------------------------------------------------------------------------------------------------
// One 1-D pass of jfdctint (CONST_BITS 13): o[0], o[4] are the plain sums, the six others carry 13 fraction bits; the caller shifts.
__device__ __forceinline__ void jpeg_fdct_1d(const long long d[8], long long o[8]) {
    const long long t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const long long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    o[0] = t10 + t11;
    o[4] = t10 - t11;
    long long z1 = (t12 + t13) * 4433;
    o[2] = z1 + t13 * 6270;
    o[6] = z1 - t12 * 15137;
    z1 = t4 + t7;
    long long z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const long long z5 = (z3 + z4) * 9633;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    o[7] = t4 * 2446 + z1 + z3;
    o[5] = t5 * 16819 + z2 + z4;
    o[3] = t6 * 25172 + z2 + z3;
    o[1] = t7 * 12299 + z1 + z4;
}

// grid ceil(blocks / 32), 256 threads: 8 lanes own one 8 x 8 block.  Lane l loads sample row l as one 8-byte vector and runs pass 1 along it, the block
// is transposed through LDS, pass 2 runs down column l and quantises it, a second transpose gives the lane coefficient row l back for one 16-byte store.
// A Y block of a 4:2:0 MCU that lies wholly beyond the component's own grid (hb x wb blocks) is libjpeg's "dummy block": no AC, and the DC of the
// block before it in the MCU's order -- its lanes transform THAT block's samples (no dependency between blocks) and drop the AC terms.
__global__ __launch_bounds__(256) void jpeg_enc_fdct_kernel(const uint8_t* __restrict__ planes, Geo g, QTables qt, int16_t* __restrict__ coefs,
                                                            uint16_t* __restrict__ qtables_out) {
    __shared__ int ws1[32][8][9];
    __shared__ short ws2[32][8][10];
    if (blockIdx.x == 0 && threadIdx.x < 128 && qtables_out) qtables_out[threadIdx.x] = qt.q[threadIdx.x >> 6][threadIdx.x & 63];
    const int l = threadIdx.x & 7, grp = threadIdx.x >> 3;
    const long long blk = (long long)blockIdx.x * 32 + grp;
    const long long total = g.nb0 + 2 * g.nbc;
    const bool valid = blk < total;
    int comp = 0, across = g.mc * g.s;
    long long li = blk;
    const uint8_t* pl = planes;
    if (blk >= g.nb0) {
        comp = blk < g.nb0 + g.nbc ? 1 : 2;
        li = blk - g.nb0 - (comp == 2 ? g.nbc : 0);
        across = g.mc;
        pl = planes + (long long)g.yw * g.yh + (comp == 2 ? (long long)g.cw * g.ch : 0);
    }
    bool dummy = false;
    if (valid) {
        int br = (int)(li / across), bc = (int)(li - (long long)br * across);
        if (comp == 0 && g.s == 2) {
            const int hb = (g.h + 7) >> 3, wb = (g.w + 7) >> 3;
            if (br >= hb) {  // a dummy bottom row: both blocks take the DC of the MCU's top-right block ...
                dummy = true;
                br -= 1;
                bc |= 1;
            }
            if (bc >= wb) {  // ... which, like any block past the right edge, is itself a dummy of the block to its left
                dummy = true;
                bc -= 1;
            }
        }
        const uint2 raw = *reinterpret_cast<const uint2*>(pl + ((long long)br * 8 + l) * (across * 8) + bc * 8);
        long long d[8], o[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[k] = (long long)((raw.x >> (8 * k)) & 255) - 128;
            d[k + 4] = (long long)((raw.y >> (8 * k)) & 255) - 128;
        }
        jpeg_fdct_1d(d, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) ws1[grp][l][k] = (int)((k & 3) == 0 ? o[k] << 2 : (o[k] + 1024) >> 11);  // |.| < 2^14
    }
    __syncthreads();
    if (valid) {
        long long d[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = ws1[grp][r][l];
        jpeg_fdct_1d(d, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int c = (int)((r & 3) == 0 ? (o[r] + 2) >> 2 : (o[r] + 16384) >> 15);  // 8 x the DCT: |c| <= 2^16
            const unsigned div = 8u * qt.q[comp ? 1 : 0][r * 8 + l];
            const unsigned m = ((unsigned)(c < 0 ? -c : c) + (div >> 1)) / div;
            ws2[grp][r][l] = (dummy && (r | l)) ? (short)0 : (short)(c < 0 ? -(int)m : (int)m);
        }
    }
    __syncthreads();
    if (valid) {
        unsigned v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (unsigned)(unsigned short)ws2[grp][l][2 * k] | ((unsigned)(unsigned short)ws2[grp][l][2 * k + 1] << 16);
        *reinterpret_cast<uint4*>(coefs + blk * 64 + l * 8) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// ---- entropy coding ------------------------------------------------------------------------------------------------------------------------------
// exclusive scan of one value per thread over a workgroup of 256 (4 waves of 64); *total: the sum.  `part` is LDS for 4 values; two barriers.
__device__ __forceinline__ unsigned block_scan_256(unsigned v, unsigned* part, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();  // (the previous use of `part` is over)
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    unsigned base = 0, sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < wave) base += part[k];
        sum += part[k];
    }
    *total = sum;
    return base + inc - v;
}

// The symbols of one block in coding order, each handed to `put(value, bit length)`; a code and its magnitude bits go as one value (<= 16 + 11 bits).
template <class Put>
__device__ __forceinline__ void jpeg_block_symbols(const int16_t* __restrict__ c, int pred, const uint32_t* __restrict__ dc, const uint32_t* __restrict__ ac,
                                                   const uint8_t* __restrict__ zz, Put put) {
    {
        const int d = (int)c[0] - pred;
        int size = 32 - __clz(d < 0 ? -d : d);  // |d| <= 2047 for what the encoder's own first half writes: size <= 11
        size = size > 11 ? 11 : size;
        const uint32_t e = dc[size];
        put((((e >> 8) << size) | ((unsigned)(d < 0 ? d - 1 : d) & ((1u << size) - 1))), (int)(e & 255) + size);
    }
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = c[zz[k]];
        if (v == 0) {
            ++run;
            continue;
        }
        while (run >= 16) {
            put(ac[0xF0] >> 8, (int)(ac[0xF0] & 255));
            run -= 16;
        }
        int size = 32 - __clz(v < 0 ? -v : v);
        size = size > 10 ? 10 : size;  // (never taken for 8-bit samples; keeps the symbol inside the table and the length inside the bound)
        const uint32_t e = ac[(run << 4) | size];
        put((((e >> 8) << size) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1))), (int)(e & 255) + size);
        run = 0;
    }
    if (run) put(ac[0] >> 8, (int)(ac[0] & 255));
}

// byte order of the stream inside a 32-bit word of memory: the word's most significant bit is the earliest bit
__device__ __forceinline__ unsigned jpeg_be32(unsigned v) { return __builtin_bswap32(v); }

// grid intervals, 256 threads.  Interval iv = it.cols MCUs of MCU row `row`, from MCU column m0 on; its blocks in coding order are numbered
// b = ml bpm + k (ml: the MCU inside the interval, k: the block inside the MCU, Y blocks in raster order, then Cb, then Cr).  The slot must be zero on entry.
__global__ __launch_bounds__(256) void jpeg_enc_entropy_kernel(const int16_t* __restrict__ coefs, Geo g, Intervals it, HuffTables ht, uint8_t* __restrict__ slots,
                                                               long long slot_bytes, int* __restrict__ raw_len) {
    __shared__ unsigned part[4];
    __shared__ uint32_t s_dc[2][12];
    __shared__ uint32_t s_ac[2][256];
    __shared__ uint8_t s_zz[64];
    for (int i = threadIdx.x; i < 24; i += 256) s_dc[i / 12][i % 12] = ht.dc[i / 12][i % 12];
    for (int i = threadIdx.x; i < 512; i += 256) s_ac[i >> 8][i & 255] = ht.ac[i >> 8][i & 255];
    if (threadIdx.x < 64) s_zz[threadIdx.x] = ht.zigzag[threadIdx.x];
    __syncthreads();
    const int iv = blockIdx.x, strm = iv / it.rows;
    const int row = (strm / it.across) * it.rows + (iv - strm * it.rows), m0 = (strm % it.across) * it.cols;
    const int n = it.cols * g.bpm;
    const int ny = g.s * g.s;
    unsigned* slot = reinterpret_cast<unsigned*>(slots + (long long)iv * slot_bytes);
    const long long slot_words = slot_bytes >> 2;
    const long long yacross = (long long)g.mc * g.s;
    unsigned long long running = 0;  // bits of the interval laid down so far
    for (int base = 0; base < n; base += 256) {
        const int b = base + (int)threadIdx.x;
        const bool valid = b < n;
        const int16_t* c = coefs;
        int pred = 0, tab = 0;
        if (valid) {
            const int ml = b / g.bpm, k = b - ml * g.bpm, m = m0 + ml;
            if (k < ny) {
                // Y block k of MCU m, and the Y block coded before it: k - 1 of this MCU, or the last one of MCU m - 1 (none at the interval's start)
                const long long at = ((long long)row * g.s + (k >> (g.s - 1))) * yacross + (long long)m * g.s + (k & (g.s - 1));
                c = coefs + at * 64;
                if (k > 0) {
                    const int kp = k - 1;
                    pred = coefs[(((long long)row * g.s + (kp >> (g.s - 1))) * yacross + (long long)m * g.s + (kp & (g.s - 1))) * 64];
                } else if (ml > 0) {
                    const int kp = ny - 1;
                    pred = coefs[(((long long)row * g.s + (kp >> (g.s - 1))) * yacross + (long long)(m - 1) * g.s + (kp & (g.s - 1))) * 64];
                }
            } else {
                tab = 1;
                c = coefs + (g.nb0 + (k - ny) * g.nbc + (long long)row * g.mc + m) * 64;
                if (ml > 0) pred = c[-64];
            }
        }
        unsigned bits = 0;
        if (valid) jpeg_block_symbols(c, pred, s_dc[tab], s_ac[tab], s_zz, [&](unsigned, int len) { bits += (unsigned)len; });
        unsigned chunk_bits;
        const unsigned long long pos0 = running + block_scan_256(bits, part, &chunk_bits);
        if (valid) {
            // a 64-bit window over the words [w, w + 1]: a value of <= 27 bits at a bit offset <= 31 always fits
            unsigned long long pos = pos0, acc = 0;
            long long w = (long long)(pos >> 5);
            jpeg_block_symbols(c, pred, s_dc[tab], s_ac[tab], s_zz, [&](unsigned value, int len) {
                acc |= (unsigned long long)value << (64 - (int)(pos & 31) - len);
                pos += (unsigned)len;
                if ((long long)(pos >> 5) != w) {
                    if (w < slot_words) atomicOr(slot + w, jpeg_be32((unsigned)(acc >> 32)));
                    acc <<= 32;
                    ++w;
                }
            });
            if ((acc >> 32) != 0 && w < slot_words) atomicOr(slot + w, jpeg_be32((unsigned)(acc >> 32)));
        }
        running += chunk_bits;
    }
    if (threadIdx.x == 0) {
        const int pad = (int)((8 - (running & 7)) & 7);  // 1-bits up to the byte
        if (pad) {
            const long long w = (long long)(running >> 5);
            const unsigned v = ((1u << pad) - 1) << (32 - (int)(running & 31) - pad);
            if (w < slot_words) atomicOr(slot + w, jpeg_be32(v));
        }
        long long bytes = (long long)((running + 7) >> 3);
        raw_len[iv] = (int)(bytes < slot_bytes ? bytes : slot_bytes);
    }
}

// grid intervals, 256 threads: len[row] = the interval's bytes + its FF bytes
__global__ __launch_bounds__(256) void jpeg_enc_count_kernel(const uint8_t* __restrict__ slots, long long slot_bytes, const int* __restrict__ raw_len,
                                                             int* __restrict__ len) {
    __shared__ unsigned part[4];
    const int row = blockIdx.x, n = raw_len[row];
    const uint4* src = reinterpret_cast<const uint4*>(slots + (long long)row * slot_bytes);
    unsigned cnt = 0;
    for (int i = threadIdx.x; i * 16 < n; i += 256) {  // (the slot is a multiple of 128 bytes: whole vectors stay inside it)
        const uint4 v = src[i];
        const unsigned wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (i * 16 + k < n && ((wd[k >> 2] >> (8 * (k & 3))) & 255) == 255) ++cnt;
    }
    unsigned total;
    block_scan_256(cnt, part, &total);
    if (threadIdx.x == 0) len[row] = n + (int)total;
}

// one workgroup: off[row] = sum of (len + 2) before it; *scan_len = the whole scan
__global__ __launch_bounds__(256) void jpeg_enc_offsets_kernel(const int* __restrict__ len, int rows, long long* __restrict__ off, long long* __restrict__ scan_len) {
    __shared__ unsigned part[4];
    long long running = 0;
    for (int base = 0; base < rows; base += 256) {
        const int i = base + (int)threadIdx.x;
        const unsigned v = i < rows ? (unsigned)len[i] + (i < rows - 1 ? 2u : 0u) : 0u;  // (256 intervals of < 2^23 bytes: the chunk's sum fits 32 bits)
        unsigned total;
        const unsigned ex = block_scan_256(v, part, &total);
        if (i < rows) off[i] = running + ex;
        running += total;
    }
    if (threadIdx.x == 0) *scan_len = running;
}

// one workgroup, a thread per tile: counts[t] = prefix + the tile's intervals + 2 per interval (RSTm, EOI behind the last); tile_off[t] = exclusive scan
// of the counts rounded up to even, tile_off[tiles] = the total; off[iv] = where interval iv's bytes start
__global__ __launch_bounds__(256) void jpeg_enc_tile_offsets_kernel(const int* __restrict__ len, int tiles, int rows, int n_prefix, long long* __restrict__ off,
                                                                    long long* __restrict__ tile_off, long long* __restrict__ counts) {
    __shared__ unsigned part[4];
    long long running = 0;
    for (int base = 0; base < tiles; base += 256) {
        const int t = base + (int)threadIdx.x;
        unsigned cnt = 0;
        if (t < tiles) {
            cnt = (unsigned)n_prefix;
            for (int r = 0; r < rows; ++r) cnt += (unsigned)len[(long long)t * rows + r] + 2u;
        }
        unsigned total;
        const unsigned ex = block_scan_256((cnt + 1u) & ~1u, part, &total);  // (256 tiles of <= 64 intervals of < 2^17 bytes: the chunk's sum fits 32 bits)
        if (t < tiles) {
            long long at = running + ex;
            tile_off[t] = at;
            counts[t] = cnt;
            at += n_prefix;
            for (int r = 0; r < rows; ++r) {
                off[(long long)t * rows + r] = at;
                at += len[(long long)t * rows + r] + 2;
            }
        }
        running += total;
    }
    if (threadIdx.x == 0) tile_off[tiles] = running;
}

// grid intervals, 256 threads, 16 source bytes per thread and step: count the FF bytes, scan, write the bytes with a 00 after every FF.  Interval `row`
// is interval row % rows of its stream: the first one puts the stream's prefix in front, every one but the last RSTm behind, the last one EOI and the
// zero byte that makes the stream's length even (ends.eoi; a stream starts at an even offset).  Nothing is written at or past scan_cap.
__global__ __launch_bounds__(256) void jpeg_enc_pack_kernel(const uint8_t* __restrict__ slots, long long slot_bytes, const int* __restrict__ raw_len,
                                                            const long long* __restrict__ off, int rows, StreamEnds ends, uint8_t* __restrict__ out,
                                                            long long scan_cap) {
    __shared__ unsigned part[4];
    const int row = blockIdx.x, n = raw_len[row], r = row % rows;
    const uint4* src = reinterpret_cast<const uint4*>(slots + (long long)row * slot_bytes);
    if (r == 0 && (int)threadIdx.x < ends.n) {
        const long long o = off[row] - ends.n + threadIdx.x;
        if (o < scan_cap) out[o] = ends.prefix[threadIdx.x];
    }
    long long at = off[row];
    for (int base = 0; base < n; base += 256 * 16) {
        const int p0 = base + (int)threadIdx.x * 16;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p0 < n) v = src[p0 >> 4];
        const unsigned wd[4] = {v.x, v.y, v.z, v.w};
        unsigned cnt = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (p0 + k < n && ((wd[k >> 2] >> (8 * (k & 3))) & 255) == 255) ++cnt;
        unsigned total;
        const unsigned ex = block_scan_256(cnt, part, &total);
        long long o = at + threadIdx.x * 16 + ex;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const unsigned byte = (wd[k >> 2] >> (8 * (k & 3))) & 255;
            if (p0 + k < n) {
                if (o < scan_cap) out[o] = (uint8_t)byte;
                ++o;
                if (byte == 255) {
                    if (o < scan_cap) out[o] = 0;
                    ++o;
                }
            }
        }
        const int took = n - base < 256 * 16 ? n - base : 256 * 16;
        at += took + total;
    }
    if (threadIdx.x == 0 && (r < rows - 1 || ends.eoi)) {
        if (at < scan_cap) out[at] = 0xFF;
        if (at + 1 < scan_cap) out[at + 1] = r < rows - 1 ? (uint8_t)(0xD0 + (r & 7)) : (uint8_t)0xD9;
        if (r == rows - 1 && (at & 1) && at + 2 < scan_cap) out[at + 2] = 0;
    }
}

int check_picture(const char* fn, int w, int h, int subsampling) {
    if (w < 1 || h < 1 || w > 32768 || h > 32768)
        return cerb_set_error(std::string(fn) + ": the picture's width and height must lie in 1 .. 32768, got " + std::to_string(w) + " x " + std::to_string(h));
    if (subsampling != 0 && subsampling != 2)
        return cerb_set_error(std::string(fn) + ": subsampling must be 0 (4:4:4) or 2 (4:2:0), got " + std::to_string(subsampling));
    return 0;
}

int launched(const char* fn) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : cerb_set_error(std::string(fn) + ": kernel launch: " + hipGetErrorString(e));
}

}  // namespace

extern "C" size_t cerb_jpeg_enc_workspace_bytes(int w, int h, int subsampling, int which) {
    if (w < 1 || h < 1 || w > 32768 || h > 32768 || (subsampling != 0 && subsampling != 2)) return 0;
    const Geo g = make_geo(w, h, subsampling);
    switch (which) {
        case 0: return planes_bytes(g);
        case 1: return (size_t)(g.nb0 + 2 * g.nbc) * 64 * sizeof(int16_t);
        case 2: return scan_ws_bytes(g);
        case 3: return scan_cap_bytes(g);
        default: return 0;
    }
}

extern "C" int cerb_jpeg_enc_coefs(const uint8_t* src, long long row_stride, int w, int h, int quality, int subsampling, int16_t* coefs, uint16_t* qtables,
                                   void* workspace, size_t ws_bytes, void* hip_stream) {
    const char* fn = "cerb_jpeg_enc_coefs";
    if (check_picture(fn, w, h, subsampling)) return 1;
    if (quality < 1 || quality > 100) return cerb_set_error(std::string(fn) + ": quality must lie in 1 .. 100, got " + std::to_string(quality));
    if (!src || !coefs || !workspace || row_stride < 3LL * w || ((uintptr_t)coefs & 15) || ((uintptr_t)workspace & 7) || ((uintptr_t)qtables & 1))
        return cerb_set_error(std::string(fn) + ": bad arguments");
    const Geo g = make_geo(w, h, subsampling);
    if (ws_bytes < planes_bytes(g))
        return cerb_set_error(std::string(fn) + ": the workspace is too small: " + std::to_string(ws_bytes) + " bytes, cerb_jpeg_enc_workspace_bytes(.., 0) = " +
                              std::to_string(planes_bytes(g)));
    QTables qt;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int a = (kQLuma[i] * scale + 50) / 100, b = (kQChroma[i] * scale + 50) / 100;
        qt.q[0][i] = (uint16_t)(a < 1 ? 1 : (a > 255 ? 255 : a));
        qt.q[1][i] = (uint16_t)(b < 1 ? 1 : (b > 255 ? 255 : b));
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const long long samples = (long long)g.cw * g.ch, blocks = g.nb0 + 2 * g.nbc;
    hipLaunchKernelGGL(jpeg_enc_planes_kernel, dim3((unsigned)((samples + 255) / 256)), dim3(256), 0, st, src, row_stride, g, (uint8_t*)workspace);
    if (launched(fn)) return 1;
    hipLaunchKernelGGL(jpeg_enc_fdct_kernel, dim3((unsigned)((blocks + 31) / 32)), dim3(256), 0, st, (const uint8_t*)workspace, g, qt, coefs, qtables);
    return launched(fn);
}

extern "C" int cerb_jpeg_enc_scan(const int16_t* coefs, int w, int h, int subsampling, void* workspace, size_t ws_bytes, uint8_t* scan_out, size_t scan_cap,
                                  long long* scan_len_dev, void* hip_stream) {
    const char* fn = "cerb_jpeg_enc_scan";
    if (check_picture(fn, w, h, subsampling)) return 1;
    if (!coefs || !workspace || !scan_out || !scan_len_dev || ((uintptr_t)coefs & 15) || ((uintptr_t)workspace & 127) || ((uintptr_t)scan_len_dev & 7))
        return cerb_set_error(std::string(fn) + ": bad arguments");
    const Geo g = make_geo(w, h, subsampling);
    if (ws_bytes < scan_ws_bytes(g))
        return cerb_set_error(std::string(fn) + ": the workspace is too small: " + std::to_string(ws_bytes) + " bytes, cerb_jpeg_enc_workspace_bytes(.., 2) = " +
                              std::to_string(scan_ws_bytes(g)));
    static const HuffTables ht = make_huff_tables();
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t slot = slot_bytes(g);
    uint8_t* slots = (uint8_t*)workspace;
    int* raw_len = (int*)(slots + (size_t)g.mr * slot);
    int* len = raw_len + g.mr;
    long long* off = (long long*)(len + g.mr);
    const hipError_t e = hipMemsetAsync(slots, 0, (size_t)g.mr * slot, st);
    if (e != hipSuccess) return cerb_set_error(std::string(fn) + ": " + hipGetErrorString(e));
    const Intervals whole{g.mr, g.mc, 1};
    const StreamEnds bare{};
    hipLaunchKernelGGL(jpeg_enc_entropy_kernel, dim3(g.mr), dim3(256), 0, st, coefs, g, whole, ht, slots, (long long)slot, raw_len);
    if (launched(fn)) return 1;
    hipLaunchKernelGGL(jpeg_enc_count_kernel, dim3(g.mr), dim3(256), 0, st, (const uint8_t*)slots, (long long)slot, (const int*)raw_len, len);
    if (launched(fn)) return 1;
    hipLaunchKernelGGL(jpeg_enc_offsets_kernel, dim3(1), dim3(256), 0, st, (const int*)len, g.mr, off, scan_len_dev);
    if (launched(fn)) return 1;
    hipLaunchKernelGGL(jpeg_enc_pack_kernel, dim3(g.mr), dim3(256), 0, st, (const uint8_t*)slots, (long long)slot, (const int*)raw_len, (const long long*)off, g.mr,
                       bare, scan_out, (long long)scan_cap);
    return launched(fn);
}

namespace {

// the tile grid of cerb_jpeg_enc_tiles, or false with `why` naming the argument
bool tile_grid(int w, int h, int tile, int subsampling, Geo* g, Intervals* it, std::string* why) {
    if (w < 1 || h < 1 || w > 32768 || h > 32768) *why = "the picture's width and height must lie in 1 .. 32768, got " + std::to_string(w) + " x " + std::to_string(h);
    else if (subsampling != 0 && subsampling != 2) *why = "subsampling must be 0 (4:4:4) or 2 (4:2:0), got " + std::to_string(subsampling);
    else if (tile < 16 || tile > 512 || tile % 16) *why = "tile must be a multiple of 16 in 16 .. 512, got " + std::to_string(tile);
    else if (w % tile || h % tile) *why = "w and h must be multiples of tile " + std::to_string(tile) + ", got " + std::to_string(w) + " x " + std::to_string(h);
    else {
        *g = make_geo(w, h, subsampling);
        *it = Intervals{tile / (8 * g->s), tile / (8 * g->s), w / tile};
        return true;
    }
    return false;
}

}  // namespace

extern "C" size_t cerb_jpeg_enc_tiles_workspace_bytes(int w, int h, int tile, int subsampling, int which) {
    Geo g;
    Intervals it;
    std::string why;
    if (!tile_grid(w, h, tile, subsampling, &g, &it, &why)) return 0;
    const size_t tiles = (size_t)(w / tile) * (h / tile);
    switch (which) {
        case 0: return tiles_ws_bytes(tiles * it.rows, slot_bytes_of((size_t)it.cols * g.bpm));
        case 1: return tiles * tile_cap_bytes(it, g.bpm);
        default: return 0;
    }
}

extern "C" int cerb_jpeg_enc_tiles(const int16_t* coefs, int w, int h, int tile, int subsampling, const uint8_t* prefix, int n_prefix, void* workspace,
                                   size_t ws_bytes, uint8_t* out, size_t out_cap, long long* offsets_dev, long long* counts_dev, void* hip_stream) {
    const char* fn = "cerb_jpeg_enc_tiles";
    Geo g;
    Intervals it;
    std::string why;
    if (!tile_grid(w, h, tile, subsampling, &g, &it, &why)) return cerb_set_error(std::string(fn) + ": " + why);
    if (n_prefix < 0 || n_prefix > 64) return cerb_set_error(std::string(fn) + ": n_prefix must lie in 0 .. 64, got " + std::to_string(n_prefix));
    if (!coefs || !workspace || !out || !offsets_dev || !counts_dev || (n_prefix && !prefix))
        return cerb_set_error(std::string(fn) + ": a null pointer (coefs, prefix, workspace, out, offsets_dev or counts_dev)");
    if (((uintptr_t)coefs & 15) || ((uintptr_t)workspace & 127) || ((uintptr_t)offsets_dev & 7) || ((uintptr_t)counts_dev & 7))
        return cerb_set_error(std::string(fn) + ": misaligned: coefs needs 16 bytes, workspace 128, offsets_dev and counts_dev 8");
    const int tiles = (w / tile) * (h / tile);
    const long long n_iv = (long long)tiles * it.rows;
    const size_t slot = slot_bytes_of((size_t)it.cols * g.bpm);
    if (ws_bytes < tiles_ws_bytes((size_t)n_iv, slot))
        return cerb_set_error(std::string(fn) + ": the workspace is too small: " + std::to_string(ws_bytes) + " bytes, cerb_jpeg_enc_tiles_workspace_bytes(.., 0) = " +
                              std::to_string(tiles_ws_bytes((size_t)n_iv, slot)));
    static const HuffTables ht = make_huff_tables();
    StreamEnds ends{};
    ends.n = n_prefix;
    ends.eoi = 1;
    for (int i = 0; i < n_prefix; ++i) ends.prefix[i] = prefix[i];
    hipStream_t st = (hipStream_t)hip_stream;
    uint8_t* slots = (uint8_t*)workspace;
    int* raw_len = (int*)(slots + (size_t)n_iv * slot);
    int* len = raw_len + n_iv;
    long long* off = (long long*)(len + n_iv);
    const hipError_t e = hipMemsetAsync(slots, 0, (size_t)n_iv * slot, st);
    if (e != hipSuccess) return cerb_set_error(std::string(fn) + ": " + hipGetErrorString(e));
    hipLaunchKernelGGL(jpeg_enc_entropy_kernel, dim3((unsigned)n_iv), dim3(256), 0, st, coefs, g, it, ht, slots, (long long)slot, raw_len);
    if (launched(fn)) return 1;
    hipLaunchKernelGGL(jpeg_enc_count_kernel, dim3((unsigned)n_iv), dim3(256), 0, st, (const uint8_t*)slots, (long long)slot, (const int*)raw_len, len);
    if (launched(fn)) return 1;
    hipLaunchKernelGGL(jpeg_enc_tile_offsets_kernel, dim3(1), dim3(256), 0, st, (const int*)len, tiles, it.rows, n_prefix, off, offsets_dev, counts_dev);
    if (launched(fn)) return 1;
    hipLaunchKernelGGL(jpeg_enc_pack_kernel, dim3((unsigned)n_iv), dim3(256), 0, st, (const uint8_t*)slots, (long long)slot, (const int*)raw_len, (const long long*)off,
                       it.rows, ends, out, (long long)out_cap);
    return launched(fn);
}
