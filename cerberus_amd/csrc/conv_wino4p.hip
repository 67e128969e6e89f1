// conv_wino4p.hip -- conv_wino4.hip's Winograd F(4x4,3x3) convolution (+ folded BN bias, ReLU) on the TILE-PLANAR layout of the decoder's
// private tensors (cerb_common.h: cerb_planar_offset).  Same arithmetic, same accumulation order, same transforms as conv_wino4.hip --
// results are bit-identical -- with the three things round 2's cycle accounting charged to the NHWC layout removed:
//   * output stage: a wave's results for one pixel position (i, j) of its 16 tiles x 16 channels ARE a contiguous 1-KiB row of the
//     planar block, so the 32 stores of an item leave straight from the registers -- no transposition through LDS, no barriers
//     (conv_wino4: 32 ds_write_b128 + 32 ds_read_b128 + 4 barriers per item, ~10 k of 70 k cycles);
//   * input path: a patch load of a wave reads 64-byte pieces that pair up into whole 128-byte lines of ONE chunk's plane (NHWC: half
//     lines whose other halves are fetched again a chunk later -- the 1.66x read amplification of round 2's PMC counters), and the
//     nine lane offsets of the 6x6 patch are kernel invariants;
//   * zero padding is data (guard ring + never-written edge pixels): no edge selects, no hang-over masks, no per-item edge bits.
// The accumulators are pinned by hand: 32 of the 36 positions live in the 256 AccVGPRs, 4 in VGPRs, through inline-asm matrix
// instructions with "a" / "v" constraints -- hipcc's own split (-amdgpu-mfma-vgpr-form) rotated 8 positions per chunk through
// v_accvgpr_read / s_nop 9 / v_accvgpr_write on the matrix pipe's lanes.
// Reference layers: models/utils/conv_layers.py:24-60 (_ConvLayer) inside models/net_desc.py:182-198 (the decoder loop).
#include <type_traits>

#include "wino_common.h"

namespace {
constexpr int NPOS = 36;
constexpr int NT = 32;                        // tiles per item: two blocks of 4x4 tiles
constexpr int CB = 16;                        // input channels per LDS pass = one plane
constexpr int V_FLOATS = NPOS * NT * CB;      // one V buffer: 72 KiB
constexpr int LDS_BYTES = 2 * V_FLOATS * 4;   // double-buffered: 144 KiB
constexpr int PLANE_BYTES = 16 * 16 * 16 * 4; // one 16-channel plane of a block
constexpr int NS = NPOS;                      // steps per chunk: one position each (one 16-byte weight load, two ds_read_b128, 8 MFMAs)
constexpr int NPOS_A = 32;                    // positions whose accumulators live in AccVGPRs (32 x 2 blocks x 4 = 256); the rest in VGPRs
// Schedule of a chunk (36 steps of 8 matrix instructions = 256 cycles each).  What round 3's counters showed (profiles/r03_*): the CU's
// vector L1 stalls IN ORDER whenever a request hits a line whose miss is still in flight (TCP_PENDING_STALL_CYCLES = 57 % of the kernel with
// the 6x6 patches loaded tile by tile: 20 of a thread's 36 patch pixels are interior pixels of its neighbours' tiles, requested a step or two
// earlier by other lanes / the other wave of the block and still on their way from HBM), and behind a stalled L1 the TA FIFOs fill and the wave
// cannot even ISSUE its next weight load (SQ_VMEM_TA_*_FIFO_FULL 8 %).  So the patch is requested in two groups that are far apart in time:
//   * the 16 INTERIOR pixels (rows / columns 1..4 = the tile's own 4x4 pixels: no other lane of this CU asks for them) as early as their
//     registers allow -- row r of the patch that has just been transformed is free after its V write at step TQ+7+r, so the interior of the
//     chunk AFTER NEXT goes out at steps TQ+8+r, four loads per step;
//   * the 20 HALO pixels (interior pixels of the neighbouring tiles, requested by their owners in the previous chunk) at steps HQ .. HQ+9 of
//     the chunk before their transform: by then the owners' misses have landed, so a halo load is an L1 / L2 hit and never waits on a
//     pending line.  Halo pixels in OTHER blocks' tiles are first touches for this CU (no pending line either).
// The weight stream is one 1-KiB load per step, WD steps ahead (smooth: bursts of 4..6 overflowed the TA FIFOs).
#ifndef P4_RING
#define P4_RING 12
#endif
constexpr int RING = P4_RING;                 // weight operand slots (NS % RING == 0: the slot of a step does not depend on the chunk)
#ifndef P4_WD
#define P4_WD 8
#endif
constexpr int WD = P4_WD;                     // weight prefetch distance in steps
#ifndef P4_PRE
#define P4_PRE P4_WD
#endif
constexpr int PRE = P4_PRE;                   // steps of the NEXT item whose weights are requested before an item's output stores
#ifndef P4_WB
#define P4_WB 1
#endif
constexpr int WB = P4_WB;                     // weight burst size in steps
#ifndef P4_TQ
#define P4_TQ 22
#endif
constexpr int TQ = P4_TQ;                     // the next chunk's patch is transformed at TQ+1 .. TQ+12, written at TQ+7 .. TQ+12
#ifndef P4_HQ
#define P4_HQ 8
#endif
constexpr int HQ = P4_HQ;                     // halo loads of the next chunk's patch: two per step at steps HQ .. HQ+9
// halo pixels in the order the vertical pass consumes their columns: column 0 (6), the top / bottom pixels of columns 1..4 (8), column 5 (6)
constexpr int halo_r(int k) { return k < 6 ? k : k < 14 ? ((k - 6) & 1 ? 5 : 0) : k - 14; }
constexpr int halo_q(int k) { return k < 6 ? 0 : k < 14 ? 1 + (k - 6) / 2 : 5; }
static_assert(NS % RING == 0 && WD + WB <= RING && NS % WB == 0 && PRE == WD && PRE <= RING, "weight ring");
static_assert(HQ + 10 <= TQ && TQ + 13 < NS && TQ + 8 + 4 <= NS, "the halo must be requested before the transform starts, the interior after its registers are free");
constexpr int BIAS_XI = 7;                    // A^T[i][1] A[1][j] = 1 for all 16 outputs: the bias enters through position (1, 1)
constexpr int CHUNK_W_BYTES = NPOS * 4 * 1024;  // packed weights of one (cout block, 16-channel chunk): 144 KiB
constexpr int WAVE_W_BYTES = NPOS * 1024;       // one wave's share: 36 steps x 1 KiB

#ifdef P4_PROF
// developer instrumentation (scripts/dev_w4pprof.py): wave P4_PROF_WAVE of workgroup P4_PROF stamps the cycle counter at every step of its third item
constexpr int PROF_BYTES = 16 * 40 * 8;
__device__ unsigned long long p4_prof_buf[16 * 40];
#ifndef P4_PROF_WAVE
#define P4_PROF_WAVE 0
#endif
#else
#ifdef P4_ABL_LDSPATCH
constexpr int PROF_BYTES = 16 * 1024;  // landing zone of the ablation's direct-to-LDS loads
#else
constexpr int PROF_BYTES = 0;
#endif
#endif

template <int I>
using IC = std::integral_constant<int, I>;
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) {
        f(IC<B>{});
        static_for<B + 1, E>(f);
    }
}

#ifndef P4_WAUX
#define P4_WAUX 0
#endif
#ifndef P4_PAUX
#define P4_PAUX 0
#endif

// The matrix instruction, with the accumulator's register file chosen by the caller.  hipcc does not model what is inside the string:
// the operands' s_waitcnt are still its own (they are ordinary register uses), the wait states are ours -- an accumulate chain needs
// none; the first reader of a finished accumulator waits through wait_mfma_results() below.
// One step = the 8 matrix instructions of one position (4 k-slots x 2 blocks) in ONE statement: hipcc pads every asm boundary whose
// neighbour touches the statement's outputs with a wait state, which eight single-instruction statements paid four times per step.
template <bool AGPR, bool ZERO>
__device__ __forceinline__ void mfma_step(f32x4& c0, f32x4& c1, const f32x4& av, const f32x4& b0, const f32x4& b1) {
#define P4_STEP_BODY(FIRST0, FIRST1)                               \
    "v_mfma_f32_16x16x4_f32 %0, %2, %6, " FIRST0 "\n\t"             \
    "v_mfma_f32_16x16x4_f32 %1, %2, %10, " FIRST1 "\n\t"            \
    "v_mfma_f32_16x16x4_f32 %0, %3, %7, %0\n\t"                     \
    "v_mfma_f32_16x16x4_f32 %1, %3, %11, %1\n\t"                    \
    "v_mfma_f32_16x16x4_f32 %0, %4, %8, %0\n\t"                     \
    "v_mfma_f32_16x16x4_f32 %1, %4, %12, %1\n\t"                    \
    "v_mfma_f32_16x16x4_f32 %0, %5, %9, %0\n\t"                     \
    "v_mfma_f32_16x16x4_f32 %1, %5, %13, %1"
#define P4_STEP_IN "v"(av[0]), "v"(av[1]), "v"(av[2]), "v"(av[3]), "v"(b0[0]), "v"(b0[1]), "v"(b0[2]), "v"(b0[3]), "v"(b1[0]), "v"(b1[1]), "v"(b1[2]), "v"(b1[3])
    if constexpr (ZERO) {
        if constexpr (AGPR) asm volatile(P4_STEP_BODY("0", "0") : "=&a"(c0), "=&a"(c1) : P4_STEP_IN);
        else asm volatile(P4_STEP_BODY("0", "0") : "=&v"(c0), "=&v"(c1) : P4_STEP_IN);
    } else {
        if constexpr (AGPR) asm volatile(P4_STEP_BODY("%0", "%1") : "+a"(c0), "+a"(c1) : P4_STEP_IN);
        else asm volatile(P4_STEP_BODY("%0", "%1") : "+v"(c0), "+v"(c1) : P4_STEP_IN);
    }
#undef P4_STEP_BODY
#undef P4_STEP_IN
}
// P4_ILV experiment: one k-slot of a step (two matrix instructions) as its own statement, so that the step's memory instructions can sit
// BETWEEN the pairs, in the shadow of a running matrix instruction, instead of in front of all eight.
//   0 (default): eight matrix instructions in one statement, everything else before them
//   1: weight load / operand reads / patch loads between the pairs;   3: and the V writes of the row transformed a step earlier
// Measured A-B-C-A-C on one box (scripts/dev_ilvab.sh): 4.27-4.38 ms (0) against 4.31-4.35 ms (3) for the two launches -- inside the
// run-to-run spread; the same rearrangement of conv_wino4b.hip's 16-instruction step: 2.71-2.74 against 2.71-2.72.  Where the instructions
// of a step sit relative to its matrix instructions is not what the wave waits for.
#ifndef P4_ILV
#define P4_ILV 0
#endif
template <bool AGPR, bool ZERO>
__device__ __forceinline__ void mfma_pair(f32x4& c0, f32x4& c1, float a, float b0, float b1) {
    if constexpr (ZERO) {
        if constexpr (AGPR) asm volatile("v_mfma_f32_16x16x4_f32 %0, %2, %3, 0\n\tv_mfma_f32_16x16x4_f32 %1, %2, %4, 0" : "=&a"(c0), "=&a"(c1) : "v"(a), "v"(b0), "v"(b1));
        else asm volatile("v_mfma_f32_16x16x4_f32 %0, %2, %3, 0\n\tv_mfma_f32_16x16x4_f32 %1, %2, %4, 0" : "=&v"(c0), "=&v"(c1) : "v"(a), "v"(b0), "v"(b1));
    } else {
        if constexpr (AGPR) asm volatile("v_mfma_f32_16x16x4_f32 %0, %2, %3, %0\n\tv_mfma_f32_16x16x4_f32 %1, %2, %4, %1" : "+a"(c0), "+a"(c1) : "v"(a), "v"(b0), "v"(b1));
        else asm volatile("v_mfma_f32_16x16x4_f32 %0, %2, %3, %0\n\tv_mfma_f32_16x16x4_f32 %1, %2, %4, %1" : "+v"(c0), "+v"(c1) : "v"(a), "v"(b0), "v"(b1));
    }
}
__device__ __forceinline__ void wait_mfma_results() { asm volatile("s_nop 15\n\ts_nop 3"); }  // 8-pass MFMA D -> VALU reader: 12 states and more

// the hardware lane id, computed where it is used (volatile: not hoisted out of the item loop): a lane-invariant kept in a register across the
// chunk loop was spilled, and its scratch reload sits in the same in-order vmcnt queue as every load the wave has in flight
__device__ __forceinline__ int fresh_lane() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// a - b as two v_pk_add_f32 with negated second operands (hipcc emits four scalar v_sub_f32 for a float4 difference); the same IEEE result
__device__ __forceinline__ f32x4 sub4(const f32x4& x, const f32x4& y) {
    f32x2 lo, hi;
    const f32x2 xl = {x[0], x[1]}, xh = {x[2], x[3]}, yl = {y[0], y[1]}, yh = {y[2], y[3]};
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(lo) : "v"(xl), "v"(yl));
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(hi) : "v"(xh), "v"(yh));
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
}

struct Blk {
    int n, by, bx;  // image, block row / column inside the launch's block grid
};
struct Item {
    int g, cb;
    Blk b0, b1;  // (no array: a dynamically indexed member would keep the whole struct in scratch, i.e. in vector registers)
    int nvalid;  // 2, or 1 when the launch has an odd number of blocks and this is the last pair (block 1 repeats block 0, stores skipped)
};
}  // namespace

// LEVEL only names the symbol: the launches of the last decoder level (<1>), of the level below it (<0>, a quarter of the work each) and of the
// two lowest levels (<2>: 8 and 16 chunks per item instead of 4) show up as separate kernels in a profiler's per-symbol statistics instead of
// one average over several launch sizes.  <3> and <4> are the encoder's residual stages (cerb_api.hip: encoder_stage_is_planar): <4> adds a
// tile-planar residual (the BasicBlock's identity) between the output transform and the ReLU floor, <3> is the block's first convolution.
template <int LEVEL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void conv_wino4p_kernel(ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr bool RES = LEVEL == 4;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int a = __builtin_amdgcn_readfirstlane(tid >> 6);  // this wave's 16 output channels of the item's 64 (= one output plane); input path: block a >> 1
    const int m = lane & 15;                                 // MFMA row (cout) / column (tile within a block)
    const int ks = lane >> 4;                                // k-slot

    const int ncb = p.Cout >> 6;
    const int nblk = p.N * p.tiles_y * p.tiles_x;  // blocks per group
    const int npair = (nblk + 1) >> 1;
    const int per_group = npair * ncb;
    const int total = per_group * p.groups;
    const int nchunk = p.Cin / CB;   // = input planes per block
    const int nplane_o = p.Cout / CB;
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    // workgroup lb takes items lb, lb + G, ...: neighbouring blocks (shared halo lines) run at the same time on one XCD and meet in its L2
    const int ISTEP = (int)gridDim.x;
    int item = lb;
    const int item_end = total;
    if (item >= item_end) return;
#ifdef P4_PROF
    const int prof_item = item + 2 * ISTEP;
#endif

    auto decode_blk = [&](int id) {
        Blk b;
        b.bx = id % p.tiles_x;
        const int r = id / p.tiles_x;
        b.by = r % p.tiles_y;
        b.n = r / p.tiles_y;
        return b;
    };
    auto decode = [&](int it) {
        Item w;
        w.g = it / per_group;
        const int L = it - w.g * per_group;
        w.cb = L % ncb;
        const int pr = L / ncb;
        w.nvalid = (2 * pr + 1 < nblk) ? 2 : 1;
        w.b0 = decode_blk(2 * pr);
        w.b1 = w.nvalid == 2 ? decode_blk(2 * pr + 1) : w.b0;
        return w;
    };
    // the block's TOP-LEFT neighbour in the guard-ringed block grid (stored index of block (by, bx) is (by + 1, bx + 1)): every patch offset is >= 0
    auto in_base = [&](int g, const Blk& b) {
#ifdef P4_ABL_PATCHL2   // ablation: every patch comes from the same few blocks (cache resident): the cost of the patch loads' HBM latency
        return reinterpret_cast<const char*>(p.in) + (((long long)(b.by & 1)) * p.pl_bxp + (b.bx & 3)) * (long long)nchunk * PLANE_BYTES;
#endif
        return reinterpret_cast<const char*>(p.in + g * p.in_gs) +
               (((long long)b.n * p.pl_byp + (b.by + p.ty_off)) * p.pl_bxp + (b.bx + p.tx_off)) * (long long)nchunk * PLANE_BYTES;
    };
    auto w_base = [&](const Item& w) {
        return reinterpret_cast<const char*>(p.wpack + w.g * p.w_gs) + (long long)w.cb * nchunk * CHUNK_W_BYTES + a * WAVE_W_BYTES;
    };

    // ---- lane invariants ---------------------------------------------------------------------------------------------------
    // input transform: thread = (tile t of the item, channel pair c); tiles 0..15 are block 0 (waves 0, 1), 16..31 block 1 (waves 2, 3)
    const int t = tid >> 3, c = tid & 7, tm = t & 15, tty = tm >> 2, ttx = tm & 3;
    const bool second = (a >> 1) != 0;
    auto mine = [&](const Item& wi) {
        Blk b;
        b.n = second ? wi.b1.n : wi.b0.n;
        b.by = second ? wi.b1.by : wi.b0.by;
        b.bx = second ? wi.b1.bx : wi.b0.bx;
        return b;
    };
    // patch element (r, q) = pixel (4 tty + r - 1, 4 ttx + q - 1) of the block: row class 0 (r = 0: pixel row 3 of the tile above, in the block
    // above when tty = 0), 1 (r = 1..4: the tile's own rows), 2 (r = 5: row 0 of the tile below); columns alike.  Nine lane offsets, for good.
    unsigned poff[3][3];
    {
        const unsigned rowblk = (unsigned)p.pl_bxp * (unsigned)nchunk * PLANE_BYTES, colblk = (unsigned)nchunk * PLANE_BYTES;
#pragma unroll
        for (int rc = 0; rc < 3; ++rc)
#pragma unroll
            for (int qc = 0; qc < 3; ++qc) {
                const int dby = (rc == 0 && tty == 0) ? 0 : (rc == 2 && tty == 3) ? 2 : 1;
                const int dbx = (qc == 0 && ttx == 0) ? 0 : (qc == 2 && ttx == 3) ? 2 : 1;
                const int ty2 = rc == 0 ? ((tty + 3) & 3) : rc == 2 ? ((tty + 1) & 3) : tty;
                const int tx2 = qc == 0 ? ((ttx + 3) & 3) : qc == 2 ? ((ttx + 1) & 3) : ttx;
                poff[rc][qc] = (unsigned)dby * rowblk + (unsigned)dbx * colblk + (unsigned)((4 * ty2 + tx2) * 64 + c * 8);
                asm volatile("" : "+v"(poff[rc][qc]));
            }
    }
    const int vw = t * CB + (((c >> 1) ^ ((tm & 8) ? 3 : 0)) << 2) + 2 * (c & 1);  // V write position (floats); position xi adds xi*NT*CB
    const int vr = m * CB + ((ks ^ ((m & 8) ? 3 : 0)) << 2);                       // V read position, block 0; block 1 adds 16*CB
    const unsigned wlane = (unsigned)lane * 16u;

    f32x2 d[6][6];  // raw patch of the NEXT chunk (two channels), transformed in place in the shadow of the matrix pipe
#ifdef P4_ABL_PREVADD
    // ablation (round 5, VERDICT r4 "missing" item 4: the decoder entry `skip + up2(prev)` fused into the first convolution's patch fetch): a 6 x 6 patch
    // of the sum needs the 4 x 4 half-resolution pixels under it as well -- 16 more 8-byte loads per thread and chunk (from lines some other patch
    // element fetches anyway: prev is a quarter of the bytes and every value serves four pixels) and 36 more packed adds.  The values are garbage; the
    // row prices the instruction issue and the 32 registers, i.e. the floor of what the fused kernel would cost over the plain one.
    f32x2 pv[4][4];
#endif
    auto issue = [&](__amdgpu_buffer_rsrc_t r, int chunk_off, int rr, int qq) __attribute__((always_inline)) {
        const int ii = rr == 0 ? 3 : rr == 5 ? 0 : rr - 1, jj = qq == 0 ? 3 : qq == 5 ? 0 : qq - 1;
#ifdef P4_ABL_PREVADD
        if ((rr == 0 || rr == 1 || rr == 3 || rr == 5) && (qq == 0 || qq == 1 || qq == 3 || qq == 5))
            pv[rr == 0 ? 0 : rr == 1 ? 1 : rr == 3 ? 2 : 3][qq == 0 ? 0 : qq == 1 ? 1 : qq == 3 ? 2 : 3] =
                buf_load2<P4_PAUX>(r, poff[rr == 0 ? 0 : rr == 5 ? 2 : 1][qq == 0 ? 0 : qq == 5 ? 2 : 1], chunk_off + ((ii ^ 1) * 4 + (jj ^ 2)) * 1024);
#endif
#ifdef P4_ABL_LDSPATCH  // ablation (round 4): what an LDS-staged raw patch would cost -- the thread reads its 36 pixels from LDS
        // (any in-range address: the values are garbage) and the workgroup's unique pixels arrive through stage_lds() below
        d[rr][qq] = *reinterpret_cast<const f32x2*>(lds + (rr * 6 + qq) * NT * CB + vw);
        return;
#endif
#ifdef P4_ABL_NOCORNER   // ablation: the four corner pixels of the patch (the loads whose lanes reach into up to four different blocks) are not requested
        if ((rr == 0 || rr == 5) && (qq == 0 || qq == 5)) return;
#endif
#ifdef P4_ABL_NOEDGE     // ablation: no halo pixel at all, the interior only
        if (rr == 0 || rr == 5 || qq == 0 || qq == 5) return;
#endif
#ifdef P4_ABL_HALOOWN   // ablation: every halo pixel is read from the lane's OWN tile (same instruction count, no lane leaves the block or its tile's row)
        d[rr][qq] = buf_load2<P4_PAUX>(r, poff[1][1], chunk_off + (ii * 4 + jj) * 1024);
        return;
#endif
#ifdef P4_ABL_CORNEROWN
        if ((rr == 0 || rr == 5) && (qq == 0 || qq == 5)) { d[rr][qq] = buf_load2<P4_PAUX>(r, poff[1][1], chunk_off + (ii * 4 + jj) * 1024); return; }
#endif
        d[rr][qq] = buf_load2<P4_PAUX>(r, poff[rr == 0 ? 0 : rr == 5 ? 2 : 1][qq == 0 ? 0 : qq == 5 ? 2 : 1], chunk_off + (ii * 4 + jj) * 1024);
    };
    // B^T x, in place (wino_common.h: wino4_bt6), with its constants pinned in registers
    f32x2 k2 = {2.f, 2.f}, k4 = {4.f, 4.f}, k5 = {5.f, 5.f};
    asm volatile("" : "+v"(k2), "+v"(k4), "+v"(k5));
#if defined(P4_ABL_PREVADD) && P4_ABL_PREVADD + 0 == 2
    // ... and the bilinear blend itself (the decoder entry is align_corners = False bilinear, net_kernels.hip: blend2 = fma(a, x, b * y)): per patch column
    // four horizontal blends of the 4 x 4 source pixels, six vertical ones, six adds -- 26 packed operations x 6 columns beside the input transform's 144
    f32x2 k75 = {0.75f, 0.75f}, k25 = {0.25f, 0.25f};
    asm volatile("" : "+v"(k75), "+v"(k25));
    auto blend = [&](const f32x2& wa, const f32x2& x, const f32x2& wb, const f32x2& y) __attribute__((always_inline)) {
        f32x2 t, r;
        asm("v_pk_mul_f32 %0, %1, %2" : "=v"(t) : "v"(wb), "v"(y));
        asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(wa), "v"(x), "v"(t));
        return r;
    };
    auto pass_v = [&](int q) __attribute__((always_inline)) {
        const int qa = q <= 1 ? 0 : q <= 3 ? 1 : 2, qb = qa + 1;
        const bool odd = (q & 1) != 0;
        f32x2 h[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = odd ? blend(k75, pv[r][qa], k25, pv[r][qb]) : blend(k25, pv[r][qa], k75, pv[r][qb]);
        const f32x2 v0 = blend(k25, h[0], k75, h[1]), v1 = blend(k75, h[1], k25, h[2]), v2 = blend(k25, h[1], k75, h[2]);
        const f32x2 v3 = blend(k75, h[2], k25, h[3]), v4 = blend(k25, h[2], k75, h[3]), v5 = blend(k75, h[2], k25, h[3]);
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(d[0][q]) : "v"(v0));
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(d[1][q]) : "v"(v1));
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(d[2][q]) : "v"(v2));
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(d[3][q]) : "v"(v3));
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(d[4][q]) : "v"(v4));
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(d[5][q]) : "v"(v5));
        wino4_bt6(d[0][q], d[1][q], d[2][q], d[3][q], d[4][q], d[5][q], k2, k4, k5);
    };
#elif defined(P4_ABL_PREVADD)
    auto pass_v = [&](int q) __attribute__((always_inline)) {
        const int qi = q == 0 ? 0 : q <= 2 ? 1 : q <= 4 ? 2 : 3;
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(d[0][q]) : "v"(pv[0][qi]));
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(d[1][q]) : "v"(pv[1][qi]));
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(d[2][q]) : "v"(pv[1][qi]));
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(d[3][q]) : "v"(pv[2][qi]));
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(d[4][q]) : "v"(pv[2][qi]));
        asm("v_pk_add_f32 %0, %0, %1" : "+v"(d[5][q]) : "v"(pv[3][qi]));
        wino4_bt6(d[0][q], d[1][q], d[2][q], d[3][q], d[4][q], d[5][q], k2, k4, k5);
    };
#else
    auto pass_v = [&](int q) __attribute__((always_inline)) { wino4_bt6(d[0][q], d[1][q], d[2][q], d[3][q], d[4][q], d[5][q], k2, k4, k5); };  // down column q
#endif
    auto pass_h = [&](int r) __attribute__((always_inline)) { wino4_bt6(d[r][0], d[r][1], d[r][2], d[r][3], d[r][4], d[r][5], k2, k4, k5); };  // along row r
    auto write_row = [&](int buf, int r) __attribute__((always_inline)) {
#pragma unroll
        for (int b = 0; b < 6; ++b) *reinterpret_cast<f32x2*>(lds + buf * V_FLOATS + (r * 6 + b) * NT * CB + vw) = d[r][b];
    };

    // ---- prologue ------------------------------------------------------------------------------------------------------------
    Item w = decode(item);
    {
        const __amdgpu_buffer_rsrc_t r0 = make_rsrc(in_base(w.g, mine(w)));
#pragma unroll
        for (int k = 0; k < 36; ++k) issue(r0, 0, k / 6, k % 6);
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) pass_v(q);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        pass_h(r);
        write_row(0, r);
    }
    {   // the interior of the SECOND chunk's patch (in the steady state the previous chunk requests it)
        const bool one = (nchunk == 1);
        const Item w1 = (one && item + ISTEP < item_end) ? decode(item + ISTEP) : w;
        const __amdgpu_buffer_rsrc_t r1 = make_rsrc(in_base(w1.g, mine(w1)));
#pragma unroll
        for (int k = 0; k < 16; ++k) issue(r1, one ? 0 : PLANE_BYTES, 1 + k / 4, 1 + k % 4);
    }
    int vbuf = 0;  // the buffer the CURRENT chunk reads; the next chunk's patch goes to vbuf ^ 1
    __syncthreads();
    __amdgpu_buffer_rsrc_t rw = make_rsrc(w_base(w));
    // Weight stream in bursts: every WB steps the operands of steps q + WD .. q + WD + WB - 1 are requested at once; the operand of step q
    // lives in slot q % RING.  Steps past the chunk's 36 belong to the next chunk, or to the next item's first chunk.
    f32x4 wq[RING];
#pragma unroll
    for (int dd = 0; dd < PRE; ++dd) wq[dd] = buf_load<P4_WAUX>(rw, wlane, dd * 1024);
    f32x4 bnext;
    auto load_bias = [&](const Item& wi) {
        const float* bias = p.bias + wi.g * p.bias_gs + wi.cb * 64 + 16 * a;
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bias), 0, 64, 0x00020000);
        bnext = buf_load<P4_WAUX>(rb, (unsigned)(fresh_lane() >> 4) * 16u, 0);
    };
    load_bias(w);

    for (;;) {
        f32x4 acc[NPOS][2];
        const bool more_items = item + ISTEP < item_end;
        const Item wnx = more_items ? decode(item + ISTEP) : w;
        const __amdgpu_buffer_rsrc_t rw_nx = more_items ? make_rsrc(w_base(wnx)) : rw;
        const char* in_cur = in_base(w.g, mine(w));
        const char* in_nx = in_base(wnx.g, mine(wnx));
        // the item that holds the chunk after next when it lies beyond this item: the next item -- or, for a one-chunk convolution, the one after
        const bool more2 = item + 2 * ISTEP < item_end;
        const Item wn2 = (nchunk == 1 && more2) ? decode(item + 2 * ISTEP) : wnx;
        const char* in_n2 = in_base(wn2.g, mine(wn2));
        auto in_nx2 = [&](int over) { return (nchunk == 1 && over >= 1) ? in_n2 : in_nx; };
        acc[BIAS_XI][0] = bnext;
        acc[BIAS_XI][1] = bnext;
#ifdef P4_PROF
        const bool prof_on = (blockIdx.x == P4_PROF) && a == P4_PROF_WAVE && (item == prof_item);
#define P4_STAMP(row, col) do { if (prof_on && lane == 0) reinterpret_cast<unsigned long long*>(lds + 2 * V_FLOATS)[(row) * 40 + (col)] = __builtin_readcyclecounter(); } while (0)
#else
#define P4_STAMP(row, col) do { } while (0)
#endif

        auto chunk = [&](auto first_tag, int ch) __attribute__((always_inline)) {
            constexpr bool FIRST = decltype(first_tag)::value;
            const bool last_ch = (ch == nchunk - 1);
            const __amdgpu_buffer_rsrc_t r_stage = make_rsrc(last_ch ? in_nx : in_cur);   // the next chunk's patch (halo loads)
            const int stage_off = (last_ch ? 0 : ch + 1) * PLANE_BYTES;
            const bool wrap2 = ch + 2 >= nchunk;                                           // the patch of the chunk after next (interior loads)
            const __amdgpu_buffer_rsrc_t r_stage2 = make_rsrc(wrap2 ? in_nx2(ch + 2 - nchunk) : in_cur);
            const int stage_off2 = (wrap2 ? (ch + 2 - nchunk) % nchunk : ch + 2) * PLANE_BYTES;
            const int wcur_off = ch * CHUNK_W_BYTES;
            const __amdgpu_buffer_rsrc_t rw_over = last_ch ? rw_nx : rw;
            const int wover_off = last_ch ? 0 : (ch + 1) * CHUNK_W_BYTES;
            const float* vsrc = lds + vbuf * V_FLOATS + vr;
            const int wbuf = vbuf ^ 1;

            f32x4 bb[2][2];  // B operands (blocks 0, 1) of step q in bb[q & 1]
            bb[0][0] = *reinterpret_cast<const f32x4*>(vsrc);
            bb[0][1] = *reinterpret_cast<const f32x4*>(vsrc + 16 * CB);
            static_for<0, NS>([&](auto Q) __attribute__((always_inline)) {
                constexpr int q = decltype(Q)::value;
                constexpr int xi = q;
                constexpr bool AG = xi < NPOS_A;
#ifdef P4_PROF
                if (ch < 15) P4_STAMP(ch, q);
#endif
#if P4_ILV
                {   // the step's memory instructions between the pairs of its matrix instructions
                    const f32x4 av = wq[q % RING];
                    const f32x4 b0 = bb[q & 1][0], b1 = bb[q & 1][1];
                    constexpr bool ZR = FIRST && xi != BIAS_XI;
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_pair<AG, ZR>(acc[xi][0], acc[xi][1], av[0], b0[0], b1[0]);
                    __builtin_amdgcn_sched_barrier(0);
#ifndef P4_ABL_NOWLOAD
                if constexpr (q % WB == 0) {
#pragma unroll
                    for (int dd = q + WD; dd < q + WD + WB; ++dd) {
                        if (FIRST && dd < PRE) continue;  // requested before the previous item's stores (or in the prologue)
                        if (dd < NS) wq[dd % RING] = buf_load<P4_WAUX>(rw, wlane, wcur_off + dd * 1024);
                        else wq[(dd - NS) % RING] = buf_load<P4_WAUX>(rw_over, wlane, wover_off + (dd - NS) * 1024);
                    }
                }
#endif
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_pair<AG, false>(acc[xi][0], acc[xi][1], av[1], b0[1], b1[1]);
                    __builtin_amdgcn_sched_barrier(0);
                if constexpr (q + 1 < NS) {
                    bb[(q + 1) & 1][0] = *reinterpret_cast<const f32x4*>(vsrc + (q + 1) * NT * CB);
                    bb[(q + 1) & 1][1] = *reinterpret_cast<const f32x4*>(vsrc + (q + 1) * NT * CB + 16 * CB);
                }
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_pair<AG, false>(acc[xi][0], acc[xi][1], av[2], b0[2], b1[2]);
                    __builtin_amdgcn_sched_barrier(0);
#if P4_ILV == 3   // the V writes of the row transformed a step ago, too (its registers take the interior loads right after)
                if constexpr (q > TQ + 7 && q <= TQ + 13) write_row(wbuf, q - TQ - 8);
#endif
#ifndef P4_ABL_NOPATCH
                if constexpr (q >= HQ && q < HQ + 10) {  // halo of the next chunk's patch, two pixels per step
                    issue(r_stage, stage_off, halo_r(2 * (q - HQ)), halo_q(2 * (q - HQ)));
                    issue(r_stage, stage_off, halo_r(2 * (q - HQ) + 1), halo_q(2 * (q - HQ) + 1));
                }
#endif
#ifndef P4_ABL_NOPATCH
                if constexpr (q >= TQ + 9 && q <= TQ + 12) {  // row q - TQ - 8 was written a step ago: its registers take the interior of the chunk after next
#pragma unroll
                    for (int u = 1; u <= 4; ++u) issue(r_stage2, stage_off2, q - TQ - 8, u);
                }
#endif
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_pair<AG, false>(acc[xi][0], acc[xi][1], av[3], b0[3], b1[3]);
                    __builtin_amdgcn_sched_barrier(0);
                // the next chunk's patch landed: B^T d B (one 1-D pass per step) and the V writes into the OTHER buffer
#ifndef P4_ABL_NOXF
                if constexpr (q > TQ && q <= TQ + 6) pass_v(q - TQ - 1);
                if constexpr (q > TQ + 6 && q <= TQ + 12) pass_h(q - TQ - 7);
#endif
#if defined(P4_ABL_VWRITE_FAKE)
                if constexpr (q > TQ + 6 && q <= TQ + 12) { if (p.N < 0) write_row(wbuf, q - TQ - 7); }  // everything upstream stays alive, nothing is written
#elif !defined(P4_ABL_NOVWRITE)
                if constexpr (P4_ILV != 3 && q > TQ + 6 && q <= TQ + 12) write_row(wbuf, q - TQ - 7);
#endif
                }
#else
#ifndef P4_ABL_NOWLOAD
                if constexpr (q % WB == 0) {
#pragma unroll
                    for (int dd = q + WD; dd < q + WD + WB; ++dd) {
                        if (FIRST && dd < PRE) continue;  // requested before the previous item's stores (or in the prologue)
                        if (dd < NS) wq[dd % RING] = buf_load<P4_WAUX>(rw, wlane, wcur_off + dd * 1024);
                        else wq[(dd - NS) % RING] = buf_load<P4_WAUX>(rw_over, wlane, wover_off + (dd - NS) * 1024);
                    }
                }
#endif
                if constexpr (q + 1 < NS) {
                    bb[(q + 1) & 1][0] = *reinterpret_cast<const f32x4*>(vsrc + (q + 1) * NT * CB);
                    bb[(q + 1) & 1][1] = *reinterpret_cast<const f32x4*>(vsrc + (q + 1) * NT * CB + 16 * CB);
                }
#ifdef P4_ABL_LDSPATCH
                if constexpr (q < P4_ABL_LDSPATCH) {  // the workgroup's share of the unique raw pixels of a chunk (2 blocks x 18 x 18 px x 16 ch = 41.5 KB = ~10
                    // 16-byte loads per thread), global -> LDS without a register: 1 KiB per wave and instruction into the 16 KiB behind the V buffers
                    const unsigned voff = (unsigned)(q * 4096 + tid * 16);
                    asm volatile("s_mov_b32 m0, %2\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voff), "s"(r_stage), "s"((unsigned)(LDS_BYTES + ((q & 3) * 4 + a) * 1024)) : "memory");
                }
#endif
#ifndef P4_ABL_NOPATCH
                if constexpr (q >= HQ && q < HQ + 10) {  // halo of the next chunk's patch, two pixels per step
                    issue(r_stage, stage_off, halo_r(2 * (q - HQ)), halo_q(2 * (q - HQ)));
                    issue(r_stage, stage_off, halo_r(2 * (q - HQ) + 1), halo_q(2 * (q - HQ) + 1));
                }
#endif
                // the next chunk's patch landed: B^T d B (one 1-D pass per step) and the V writes into the OTHER buffer
#ifndef P4_ABL_NOXF
                if constexpr (q > TQ && q <= TQ + 6) pass_v(q - TQ - 1);
                if constexpr (q > TQ + 6 && q <= TQ + 12) pass_h(q - TQ - 7);
#endif
#if defined(P4_ABL_VWRITE_FAKE)
                if constexpr (q > TQ + 6 && q <= TQ + 12) { if (p.N < 0) write_row(wbuf, q - TQ - 7); }  // everything upstream stays alive, nothing is written
#elif !defined(P4_ABL_NOVWRITE)
                if constexpr (q > TQ + 6 && q <= TQ + 12) write_row(wbuf, q - TQ - 7);
#endif
#ifndef P4_ABL_NOPATCH
                if constexpr (q >= TQ + 9 && q <= TQ + 12) {  // row q - TQ - 8 was written a step ago: its registers take the interior of the chunk after next
#pragma unroll
                    for (int u = 1; u <= 4; ++u) issue(r_stage2, stage_off2, q - TQ - 8, u);
                }
#endif
                __builtin_amdgcn_sched_barrier(0);
                const f32x4 av = wq[q % RING];
                const f32x4 b0 = bb[q & 1][0], b1 = bb[q & 1][1];
                mfma_step<AG, FIRST && xi != BIAS_XI>(acc[xi][0], acc[xi][1], av, b0, b1);
#endif
                __builtin_amdgcn_sched_barrier(0);
            });
#ifndef P4_ABL_NOBAR
            __syncthreads();  // everybody has read this chunk's V and written the next one's
#endif
            vbuf ^= 1;
        };
        chunk(std::true_type{}, 0);
        for (int ch = 1; ch < nchunk; ++ch) chunk(std::false_type{}, ch);

        // ---- output transform A^T M A, entirely in registers; lane (m, ks): tile m of each block, channels 4 ks .. + 3 of the wave's 16 -------
        // vmcnt retires in order across loads AND stores: everything the next item needs during its first PRE steps is requested here, before
        // this item's stores enter the queue (its steps 0 .. WD-1 went out during the last chunk).
#pragma unroll
        for (int dd = WD; dd < PRE; ++dd) wq[dd % RING] = buf_load<P4_WAUX>(rw_nx, wlane, dd * 1024);
        load_bias(wnx);
        P4_STAMP(15, 0);
        wait_mfma_results();
#ifdef P4_ABL_NOOUT
        if (acc[0][0][0] == 1.2345e-30f)
#endif
        {
            // the ReLU floor as a SCALAR made here, per item: hipcc had put this kernel invariant in a vector register at kernel start, spilled it,
            // and reloaded it in the middle of the output stage -- behind an s_waitcnt vmcnt(0) that drained every load and every store in flight
            int relu_s = p.relu;
            asm volatile("" : "+s"(relu_s));
            const float floor_ = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(relu_s ? 0 : (int)0xff7fffff));
            // the lane's place in a 1-KiB pixel-position row, recomputed per item from the hardware lane id: a value kept in a register across the
            // chunk loop instead was spilled, and its scratch reload -- in the same in-order vmcnt queue as everything else -- drained the queue here
            const int lane_o = fresh_lane();
            const int m_o = lane_o & 15;
            const unsigned olane = (unsigned)(m_o * 64 + (lane_o >> 4) * 16);  // lane (tile m, channel quad ks)
#pragma unroll
            for (int tb = 0; tb < 2; ++tb) {
                const Blk bo = tb ? w.b1 : w.b0;
                if (tb == 1 && w.nvalid == 1) continue;  // the pair's second block repeats the first: nothing to store
                const int by_abs = bo.by + p.ty_off, bx_abs = bo.bx + p.tx_off;
                const long long origin = p.out_gs * w.g + ((((long long)bo.n * p.pl_byp + by_abs + 1) * p.pl_bxp + bx_abs + 1) * nplane_o + w.cb * 4 + a) * (long long)(PLANE_BYTES / 4);
                const __amdgpu_buffer_rsrc_t r_out = __builtin_amdgcn_make_buffer_rsrc(p.out + origin, 0, PLANE_BYTES, 0x00020000);
                const bool partial = (by_abs * BLK + BLK > p.Ho) || (bx_abs * BLK + BLK > p.Wo);
                // The residual has the output's geometry and plane count: the 1-KiB row a wave is about to store is the row it reads, at the same lane
                // offset (a masked store's out-of-range offset masks the load too: it returns zeros).  Every element is read by the lane that writes
                // it, before it writes it, so the output may be written over the residual.  Two pixel rows (eight loads, 32 registers) are in flight
                // at a time -- rows 0 and 1 go out ahead of the vertical pass, row i + 2 behind row i's stores: all sixteen at once (64 registers on
                // top of T's 96) made hipcc spill lane invariants of the CHUNK loop, with their reloads behind s_waitcnt vmcnt(0) in the matrix phase.
                f32x4 rs[RES ? 4 : 1][RES ? 4 : 1];
                auto load_res = [&](int i) __attribute__((always_inline)) {
                    if constexpr (RES) {
                        const int res_y = p.Ho - by_abs * BLK - 4 * (m_o >> 2), res_x = p.Wo - bx_abs * BLK - 4 * (m_o & 3);
                        const __amdgpu_buffer_rsrc_t r_res = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.resid) + (origin - p.out_gs * w.g + p.resid_gs * w.g), 0, PLANE_BYTES, 0x00020000);
#pragma unroll
                        for (int j = 0; j < 4; ++j) rs[i][j] = buf_load<0>(r_res, (!partial || (i < res_y && j < res_x)) ? olane : 0x80000000u, (i * 4 + j) * 1024);
                    }
                };
                load_res(0);
                load_res(1);
                // vertical pass: T[i][b] = sum_a A^T[i][a] M[a][b]
                f32x4 T[4][6];
#pragma unroll
                for (int b = 0; b < 6; ++b) {
                    const f32x4 m0 = acc[0 * 6 + b][tb], m1 = acc[1 * 6 + b][tb], m2 = acc[2 * 6 + b][tb], m3 = acc[3 * 6 + b][tb],
                                m4 = acc[4 * 6 + b][tb], m5 = acc[5 * 6 + b][tb];
#ifdef P4_ABL_NOVPASS  // ablation (round 5): the vertical pass costs nothing -- the upper bound of hiding it under the last chunk
                    T[0][b] = m0; T[1][b] = m1 + m5; T[2][b] = m2 + m3; T[3][b] = m4;
#else
                    const f32x4 s1 = m1 + m2, d1 = sub4(m1, m2), s2 = m3 + m4, d2 = sub4(m3, m4);
                    T[0][b] = m0 + s1 + s2;
                    T[1][b] = d1 + 2.f * d2;
                    T[2][b] = s1 + 4.f * s2;
                    T[3][b] = (d1 + 8.f * d2) + m5;
#endif
                }
                const int rem_y = p.Ho - by_abs * BLK - 4 * (m_o >> 2), rem_x = p.Wo - bx_abs * BLK - 4 * (m_o & 3);  // partial blocks: rows / columns of this lane's tile inside the image
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 s1 = T[i][1] + T[i][2], d1 = sub4(T[i][1], T[i][2]), s2 = T[i][3] + T[i][4], d2 = sub4(T[i][3], T[i][4]);
                    f32x4 y[4];
                    y[0] = T[i][0] + s1 + s2;
                    y[1] = d1 + 2.f * d2;
                    y[2] = s1 + 4.f * s2;
                    y[3] = (d1 + 8.f * d2) + T[i][5];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        f32x4 o = y[j];
                        if constexpr (RES) o = o + rs[i][j];
                        o[0] = fmaxf(o[0], floor_);
                        o[1] = fmaxf(o[1], floor_);
                        o[2] = fmaxf(o[2], floor_);
                        o[3] = fmaxf(o[3], floor_);
                        // pixels of an edge block beyond the image are never written: they stay zero (the next convolution's padding)
#ifdef P4_ABL_STOREOOB   // ablation: every store is issued and dropped by the descriptor's bounds check
                        const unsigned vo = 0x80000000u | olane;
#else
                        const unsigned vo = (!partial || (i < rem_y && j < rem_x)) ? olane : 0x80000000u;
#endif
#ifndef P4_ABL_NOSTORE
                        buf_store(o, r_out, vo, (i * 4 + j) * 1024);
#else
                        if (o[0] == 1.2345e-30f) buf_store(o, r_out, vo, (i * 4 + j) * 1024);
#endif
                    }
                    if constexpr (RES) {
                        if (i + 2 < 4) load_res(i + 2);
                    }
                }
            }
        }
#ifdef P4_PROF
        P4_STAMP(15, 1);
        if (prof_on) {
            __builtin_amdgcn_s_waitcnt(0);
            P4_STAMP(15, 2);
            __builtin_amdgcn_s_waitcnt(0);
            for (int i = lane; i < 16 * 40; i += 64) p4_prof_buf[i] = reinterpret_cast<unsigned long long*>(lds + 2 * V_FLOATS)[i];
        }
#endif
        if (!more_items) break;
        item += ISTEP;
        w = wnx;
        rw = rw_nx;
    }
}

hipError_t cerb_launch_wino4p(ConvParams p, hipStream_t st) {
    if (p.Cin % CB || p.Cout % 64 || (p.resid != nullptr) != (p.level_tag == 4) || p.pl_byp < 3 || p.pl_bxp < 3 || p.H != p.Ho || p.W != p.Wo) return hipErrorInvalidValue;
    const long long nblk = wino4_block_grid(p);
    if (p.pl_byp != (p.Ho + BLK - 1) / BLK + 2 || p.pl_bxp != (p.Wo + BLK - 1) / BLK + 2) return hipErrorInvalidValue;
    const long long items = (long long)p.groups * ((nblk + 1) / 2) * (p.Cout / 64);
    const int tag = p.level_tag >= 2 && p.level_tag <= 4 ? p.level_tag : p.level_tag ? 1 : 0;
    auto kern = tag == 4 ? conv_wino4p_kernel<4> : tag == 3 ? conv_wino4p_kernel<3> : tag == 2 ? conv_wino4p_kernel<2> : tag ? conv_wino4p_kernel<1> : conv_wino4p_kernel<0>;
    static bool attr_done[5][64] = {};
    return wino4_launch(kern, attr_done[tag], items, LDS_BYTES + PROF_BYTES, p, st);
}

#ifdef P4_PROF
extern "C" int cerb_w4p_prof_read(unsigned long long* dst) { return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(p4_prof_buf), sizeof(unsigned long long) * 16 * 40); }
#endif
