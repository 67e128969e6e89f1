// wino_common.h -- what the Winograd convolution kernels (conv_wino.hip, conv_wino4.hip, conv_wino4b.hip, conv_wino4p.hip) share: buffer-resource
// addressing (conv_igemm.hip includes this header for that part only), the 1-D passes of the F(4x4, 3x3) transforms, the block output stage of
// the two NHWC F(4x4) kernels and their launchers' set-up.  Everything device code calls is __device__ __forceinline__: the kernels keep their
// arrays in registers only while nothing that takes them by reference is compiled out of line (tests/test_isa_hazard.py).
#pragma once
#include "cerb_common.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Buffer-resource addressing: address = descriptor base (4 SGPRs, built by the scalar unit per item) + per-lane 32-bit byte offset (VGPR)
// + uniform byte offset (SGPR) -- no VALU instruction per access.  AUX is the instruction's cache-policy immediate (the units' *_AUX switches).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, -1, 0x00020000);  // raw buffer, no range clipping
}
// 2 GiB of range, so that a lane offset of 0x80000000 is out of range and the hardware returns zeros / drops the store (zero padding of the
// image border without a single VALU instruction)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc_lim(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
}
template <int AUX = 0>
__device__ __forceinline__ f32x4 buf_load(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, soff, AUX));
}
template <int AUX = 0>
__device__ __forceinline__ f32x2 buf_load2(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, soff, AUX));
}
template <int AUX = 0>
__device__ __forceinline__ void buf_store(f32x4 v, __amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)voff, soff, AUX);
    // gfx950 hazard hipcc (ROCm 7.2) does not pad: buffer_store_dwordx4 whose soffset is an SGPR, followed directly by a VALU
    // write of its data VGPRs, stores corrupted data (the compiler only inserts wait states for the immediate-soffset form).
    // Found as run-to-run differing outputs; two wait states pinned behind the store cure it (scripts/dev_wrace.sh,
    // tests/test_isa_hazard.py).
    asm volatile("s_nop 1");
    __builtin_amdgcn_sched_barrier(0);
}

// ---- F(4x4, 3x3), points (0, 1, -1, 2, -2, inf) -------------------------------------------------------------------------------------------
// Input transform B^T x, in place: 12 packed operations.  Written as v_pk_fma_f32 / v_pk_add_f32 by hand: hipcc (ROCm 7.2) scalarises vector
// subtractions and multiplies by negative literals (116 v_fma_f32 + 44 v_add_f32 + 64 packed instructions per chunk instead of 144 packed
// ones), and every VALU instruction of these waves is a matrix-pipe cycle lost (one wave per SIMD).  k2, k4, k5 = the constants 2, 4, 5 in
// both halves, pinned in vector registers by the caller (asm volatile("" : "+v"(k)): the compiler would rematerialise them per use).
__device__ __forceinline__ void wino4_bt6(f32x2& x0, f32x2& x1, f32x2& x2, f32x2& x3, f32x2& x4, f32x2& x5, const f32x2& k2, const f32x2& k4,
                                          const f32x2& k5) {
#ifdef W4_C_XF
    const f32x2 t0 = x4 - 4.f * x2, t1 = x3 - 4.f * x1;
    const f32x2 u0 = x4 - x2, u1 = x3 - x1;
    x0 = (4.f * x0 + x4) - 5.f * x2;
    x5 = (4.f * x1 + x5) - 5.f * x3;
    x1 = t0 + t1;
    x2 = t0 - t1;
    x3 = u0 + 2.f * u1;
    x4 = u0 - 2.f * u1;
#else
    f32x2 t0, t1, u0, u1;
    asm("v_pk_fma_f32 %6, %2, %11, %4 neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"   // t0 = x4 - 4 x2
        "v_pk_fma_f32 %7, %1, %11, %3 neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"   // t1 = x3 - 4 x1
        "v_pk_add_f32 %8, %4, %2 neg_lo:[0,1] neg_hi:[0,1]\n\t"            // u0 = x4 - x2
        "v_pk_add_f32 %9, %3, %1 neg_lo:[0,1] neg_hi:[0,1]\n\t"            // u1 = x3 - x1
        "v_pk_fma_f32 %0, %0, %11, %4\n\t"                                  // x0 = 4 x0 + x4
        "v_pk_fma_f32 %5, %1, %11, %5\n\t"                                  // x5 = 4 x1 + x5
        "v_pk_fma_f32 %0, %2, %12, %0 neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"   // x0 -= 5 x2
        "v_pk_fma_f32 %5, %3, %12, %5 neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"   // x5 -= 5 x3
        "v_pk_add_f32 %1, %6, %7\n\t"                                       // x1 = t0 + t1
        "v_pk_add_f32 %2, %6, %7 neg_lo:[0,1] neg_hi:[0,1]\n\t"            // x2 = t0 - t1
        "v_pk_fma_f32 %3, %9, %10, %8\n\t"                                  // x3 = u0 + 2 u1
        "v_pk_fma_f32 %4, %9, %10, %8 neg_lo:[1,0,0] neg_hi:[1,0,0]"         // x4 = u0 - 2 u1
        : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "=&v"(t0), "=&v"(t1), "=&v"(u0), "=&v"(u1)
        : "v"(k2), "v"(k4), "v"(k5));
#endif
}

// Output transform, one 1-D pass y = A^T m (both passes of A^T M A are this one).  The summation order is part of the kernels' contract: the
// F(4x4) kernels are tested bit for bit against each other.  The outputs may be LDS locations: each is written as soon as it is known.
__device__ __forceinline__ void wino4_at4(f32x4 m0, f32x4 m1, f32x4 m2, f32x4 m3, f32x4 m4, f32x4 m5, f32x4& y0, f32x4& y1, f32x4& y2, f32x4& y3) {
    const f32x4 s1 = m1 + m2, d1 = m1 - m2, s2 = m3 + m4, d2 = m3 - m4;
    y0 = m0 + s1 + s2;
    y1 = d1 + 2.f * d2;
    y2 = s1 + 4.f * s2;
    y3 = (d1 + 8.f * d2) + m5;
}

// ---- block output stage of the NHWC F(4x4) kernels (conv_wino4.hip, conv_wino4b.hip) ------------------------------------------------------------
constexpr int BLK = 16;  // a block is 16x16 output pixels = 4x4 tiles of 4x4
constexpr int OPX = 68;  // output staging: floats per pixel (64 channels + 4: bank skew); a block needs 256 * OPX + 16 floats of LDS
struct Wino4Block {
    int g, cb, n, by, bx;  // group, block of 64 output channels, image, block row / column inside the launch's block grid (PACKED: n = the packed block)
};

// The workgroup's four waves finish ONE block x 64 output channels: wave a holds M = acc(0) .. acc(35) for 16 channels, lane (m, ks) = tile m of the
// block, channels 4 ks .. + 3.  A^T M A is additions in registers.  A wave's results are 64-byte pieces (16 channels) of pixels 4 apart: stored
// directly, one instruction touches 16 partial cache lines and takes ~300 cycles to issue with the matrix pipe idle.  The waves therefore transpose
// the block through `stg` (a V buffer the last chunk has finished with) into [pixel][64 channels] and store whole pixel rows -- 1 KiB contiguous
// (4 pixels x 256 bytes) per instruction -- with residual, ReLU floor and, for training, the BatchNorm partials of ConvParams::bn_part through `bnred`
// (4 * 16 * 8 doubles of LDS, 16-byte aligned): STATS 1 = (sum, sum of squares) of the outputs, summed in double; STATS 2 = the BatchNorm-backward sums (ConvParams::bst_*).
// PACKED (conv_wino4b.hip): the block's 16 tiles are tiles 16 n .. 16 n + 15 of the group, placed by pk_decode(tile, n, ty, tx); rows leave per tile.
// dead: nothing is stored or counted (the repeated second block of conv_wino4.hip's last pair); every wave still meets both barriers.
// lane_o: the lane id, made opaque per item by the caller (keeps what derives from it out of the matrix phase's register budget).
// stamp(k): profiling probe, compiled out unless the unit defines W4_PROF -- 0 vertical pass done, 1 staged, 2 / 4 behind the barriers, 3 stored.
template <bool HAS_RES, int STATS, bool PACKED, int LD_AUX, int ST_AUX, class Acc, class PkDecode, class Stamp>
__device__ __forceinline__ void wino4_store_block(const ConvParams& p, float* stg, float* bnred, int a, int lane_o, const Wino4Block& w, bool dead,
                                                  Acc&& acc, PkDecode&& pk_decode, Stamp&& stamp) {
    const int mo = lane_o & 15, kso = lane_o >> 4;
    // write side: lane (tile mo, channel quad kso) owns pixels (4 ty + i, 4 tx + j); pixel stride 68 floats, 4 floats of skew per tile row
    const int sw = ((64 * (mo >> 2) + 4 * (mo & 3)) * OPX + 4 * (mo >> 2) + 16 * a + 4 * kso);
    // read side: wave a stores pixel rows 4 a .. 4 a + 3; lane = (pixel lane_o >> 4 of a group of four, 16-byte piece lane_o & 15)
    const int sr = ((64 * a + (lane_o >> 4)) * OPX + 4 * a + 4 * (lane_o & 15));
    const int orow = p.Wo * p.Cout * 4, opix = p.Cout * 4;
    const unsigned ooff = (unsigned)((((PACKED ? 0 : 4 * a * p.Wo) + (lane_o >> 4)) * p.Cout + 4 * (lane_o & 15)) * 4);
    const float floor_ = p.relu ? 0.f : -3.402823466e38f;
    const unsigned span = PACKED ? (unsigned)((long long)p.N * p.Ho * p.Wo * p.Cout * 4) : (unsigned)(BLK * p.Wo * p.Cout * 4);
    const int by0 = (w.by + p.ty_off) * BLK, bx0 = (w.bx + p.tx_off) * BLK;
    const long long origin = PACKED ? (long long)w.cb * 64 : (((long long)w.n * p.Ho + by0) * p.Wo + bx0) * p.Cout + w.cb * 64;  // floats, uniform
    const __amdgpu_buffer_rsrc_t r_out = __builtin_amdgcn_make_buffer_rsrc(p.out + w.g * p.out_gs + origin, 0, span, 0x00020000);
    const bool partial = !PACKED && ((by0 + BLK > p.Ho) || (bx0 + BLK > p.Wo));
    // PACKED: this wave stores tiles 4 a .. 4 a + 3 of the item; a tile's byte offset in the group's tensor joins the lane's own offset
    unsigned toff[4] = {0u, 0u, 0u, 0u};
    bool tvalid[4] = {true, true, true, true};
    if (PACKED) {
#pragma unroll
        for (int x4 = 0; x4 < 4; ++x4) {
            const int T = w.n * 16 + 4 * a + x4;
            tvalid[x4] = T < p.pk_ntile;
            int n, ty, tx;
            pk_decode(tvalid[x4] ? T : 0, n, ty, tx);
            toff[x4] = (unsigned)(((n * p.Ho + 4 * ty) * p.Wo + 4 * tx) * p.Cout * 4);
        }
    }
    // vertical pass: T[i][b] = sum_a A^T[i][a] M[a][b]
    f32x4 T[4][6];
#pragma unroll
    for (int b = 0; b < 6; ++b) wino4_at4(acc(0 * 6 + b), acc(1 * 6 + b), acc(2 * 6 + b), acc(3 * 6 + b), acc(4 * 6 + b), acc(5 * 6 + b), T[0][b], T[1][b], T[2][b], T[3][b]);
    stamp(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float* y = stg + sw + 16 * i * OPX;
        wino4_at4(T[i][0], T[i][1], T[i][2], T[i][3], T[i][4], T[i][5], *reinterpret_cast<f32x4*>(y), *reinterpret_cast<f32x4*>(y + OPX),
                  *reinterpret_cast<f32x4*>(y + 2 * OPX), *reinterpret_cast<f32x4*>(y + 3 * OPX));
    }
    stamp(1);
    __syncthreads();
    stamp(2);
    // 16 groups of four pixels per wave: row 4 a + (k >> 2), pixels 4 (k & 3) .. + 3
    unsigned vo[4];
#pragma unroll
    for (int x4 = 0; x4 < 4; ++x4) {
        const bool ok = !dead && (PACKED ? tvalid[x4] : (!partial || (bx0 + 4 * x4 + (lane_o >> 4) < p.Wo)));
        vo[x4] = ok ? ooff + toff[x4] : 0x80000000u;  // out-of-range offsets: the hardware drops the store / returns 0
    }
    f32x4 res[16];
    if (HAS_RES) {
        const __amdgpu_buffer_rsrc_t r_res =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.resid + w.g * p.resid_gs + origin), 0, span, 0x00020000);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const bool rowok = !partial || (by0 + 4 * a + (k >> 2) < p.Ho);
            res[k] = buf_load<LD_AUX>(r_res, rowok ? vo[k & 3] : 0x80000000u, (k >> 2) * orow + (PACKED ? 0 : 4 * (k & 3) * opix));
        }
    }
    // (requested here, behind the staging barrier; requested before the output transform instead: no faster, and one instantiation of conv_wino4b spilled)
    f32x4 yv[STATS == 2 ? 16 : 1], bm, brs, bga, bbe;  // STATS 2: the BatchNorm's input at this lane's pixels, its parameters for this lane's four channels
    if constexpr (STATS == 2) {
        const __amdgpu_buffer_rsrc_t r_y =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bst_y + w.g * p.bst_y_gs + origin), 0, span, 0x00020000);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const bool rowok = !partial || (by0 + 4 * a + (k >> 2) < p.Ho);
            yv[k] = buf_load<LD_AUX>(r_y, rowok ? vo[k & 3] : 0x80000000u, (k >> 2) * orow + (PACKED ? 0 : 4 * (k & 3) * opix));
        }
        const int pc = w.g * p.Cout + w.cb * 64 + 4 * (lane_o & 15);
        bm = *reinterpret_cast<const f32x4*>(p.bst_mean + pc);
        brs = *reinterpret_cast<const f32x4*>(p.bst_rstd + pc);
        bga = *reinterpret_cast<const f32x4*>(p.bst_gamma + pc);
        bbe = *reinterpret_cast<const f32x4*>(p.bst_beta + pc);
    }
    f32x4 bts = {0.f, 0.f, 0.f, 0.f}, btq = {0.f, 0.f, 0.f, 0.f};  // STATS 2: this lane's 16 pixels x 4 channels
    // STATS 1: (sum, sum of squares) in double from the first addition on -- the partial rows are doubles, and a float sum over a block's 256 pixels put the
    // variance 2e-7 .. 4e-7 (relative) from the float64 statistics of the very output stored here, up to 5.5 x torch's float32 error
    // (tests/test_conv_forward_parity_gpu.py); `bnred` then holds [wave][channel quad][4 sums, 4 sums of squares] DOUBLES
    double dts[4] = {0.0, 0.0, 0.0, 0.0}, dtq[4] = {0.0, 0.0, 0.0, 0.0};
    double* bnred_d = reinterpret_cast<double*>(bnred);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        f32x4 o = *reinterpret_cast<const f32x4*>(stg + sr + (16 * (k >> 2) + 4 * (k & 3)) * OPX);
        if (HAS_RES) o = o + res[k];
        o[0] = fmaxf(o[0], floor_);
        o[1] = fmaxf(o[1], floor_);
        o[2] = fmaxf(o[2], floor_);
        o[3] = fmaxf(o[3], floor_);
        const bool rowok = !partial || (by0 + 4 * a + (k >> 2) < p.Ho);
        if constexpr (STATS == 1) {
            if (rowok && vo[k & 3] != 0x80000000u) {  // pixels inside the image only
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double od = (double)o[e];
                    dts[e] += od;
                    dtq[e] = fma(od, od, dtq[e]);
                }
            }
        }
        if constexpr (STATS == 2) {
            if (rowok && vo[k & 3] != 0x80000000u) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {  // the mask by the ONE expression every BatchNorm kernel uses (train_kernels.hip: bn_out): identical ReLU masks
                    const float yy = yv[k][e];
                    const float z = __fmaf_rn(yy - bm[e], brs[e] * bga[e], bbe[e]);
                    const float g = z > 0.f ? o[e] : 0.f;
                    bts[e] += g;
                    btq[e] = fmaf(g, (yy - bm[e]) * brs[e], btq[e]);
                }
            }
        }
#ifdef W4_ABL_NOSTORE
        if (o[0] == 1.2345e-30f)
#endif
        buf_store<ST_AUX>(o, r_out, rowok ? vo[k & 3] : 0x80000000u, (k >> 2) * orow + (PACKED ? 0 : 4 * (k & 3) * opix));
    }
    if constexpr (STATS == 1) {  // the four lanes that hold a channel quad, then (behind the barrier) the four waves = the block's 256 pixels
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            dts[e] += __shfl_xor(dts[e], 16);
            dts[e] += __shfl_xor(dts[e], 32);
            dtq[e] += __shfl_xor(dtq[e], 16);
            dtq[e] += __shfl_xor(dtq[e], 32);
        }
        if (lane_o < 16) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bnred_d[(a * 16 + lane_o) * 8 + e] = dts[e];
                bnred_d[(a * 16 + lane_o) * 8 + 4 + e] = dtq[e];
            }
        }
    }
    if constexpr (STATS == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bts[e] += __shfl_xor(bts[e], 16);
            bts[e] += __shfl_xor(bts[e], 32);
            btq[e] += __shfl_xor(btq[e], 16);
            btq[e] += __shfl_xor(btq[e], 32);
        }
        if (lane_o < 16) {
            *reinterpret_cast<f32x4*>(bnred + (a * 16 + lane_o) * 8) = bts;
            *reinterpret_cast<f32x4*>(bnred + (a * 16 + lane_o) * 8 + 4) = btq;
        }
    }
    stamp(3);
    __syncthreads();  // the staging buffer is a V buffer: the item's next block, then the next item's chunks, write it
    stamp(4);
    if constexpr (STATS) {
        if (a == 0 && lane_o < 16 && !dead && p.bn_part) {
            const long long blk = PACKED ? (long long)w.n : ((long long)w.n * p.tiles_y + w.by) * p.tiles_x + w.bx;
            double* dst = p.bn_part + (((long long)w.g * p.bn_bpg + blk) * p.Cout + w.cb * 64 + 4 * lane_o) * 2;
            if constexpr (STATS == 1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    dst[2 * e] = ((bnred_d[lane_o * 8 + e] + bnred_d[(16 + lane_o) * 8 + e]) + bnred_d[(32 + lane_o) * 8 + e]) + bnred_d[(48 + lane_o) * 8 + e];
                    dst[2 * e + 1] = ((bnred_d[lane_o * 8 + 4 + e] + bnred_d[(16 + lane_o) * 8 + 4 + e]) + bnred_d[(32 + lane_o) * 8 + 4 + e]) + bnred_d[(48 + lane_o) * 8 + 4 + e];
                }
            }
            if constexpr (STATS == 2) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    dst[2 * e] = (double)(((bnred[lane_o * 8 + e] + bnred[(16 + lane_o) * 8 + e]) + bnred[(32 + lane_o) * 8 + e]) + bnred[(48 + lane_o) * 8 + e]);
                    dst[2 * e + 1] = (double)(((bnred[lane_o * 8 + 4 + e] + bnred[(16 + lane_o) * 8 + 4 + e]) + bnred[(32 + lane_o) * 8 + 4 + e]) + bnred[(48 + lane_o) * 8 + 4 + e]);
                }
            }
        }
    }
}

// ---- host: launcher set-up of the F(4x4) kernels -------------------------------------------------------------------------------------------------
// The launch's grid of 16x16 blocks (ConvParams::tiles_* count BLOCKS here), cut down to the region of interest if there is one.  -> blocks per group
static inline long long wino4_block_grid(ConvParams& p) {
    p.tiles_x = (p.Wo + BLK - 1) / BLK;
    p.tiles_y = (p.Ho + BLK - 1) / BLK;
    p.ty_off = p.tx_off = 0;
    if (p.roi_y1 > p.roi_y0 && p.roi_x1 > p.roi_x0) {
        p.ty_off = p.roi_y0 / BLK;
        p.tx_off = p.roi_x0 / BLK;
        p.tiles_y = (p.roi_y1 + BLK - 1) / BLK - p.ty_off;
        p.tiles_x = (p.roi_x1 + BLK - 1) / BLK - p.tx_off;
    }
    return (long long)p.N * p.tiles_x * p.tiles_y;
}
// which BatchNorm partials the output stage leaves (the kernels' STATS): 0 none, 1 training forward, 2 training backward
static inline int wino4_stats(const ConvParams& p) { return p.bn_part == nullptr ? 0 : (p.bst_y ? 2 : 1); }
// persistent launch, one workgroup of 4 waves per CU, with the kernel's dynamic LDS size raised once per device (attr_done: one row per instantiation)
template <class K>
static inline hipError_t wino4_launch(K kern, bool (&attr_done)[64], long long items, int lds_bytes, const ConvParams& p, hipStream_t st) {
    if (cerb_attr_needed(attr_done)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (e != hipSuccess) return e;
    }
    const long long grid = items < 256 ? items : 256;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds_bytes, st, p);
    return hipGetLastError();
}
