// conv_wino4.hip -- 3x3 stride-1 convolution (+ folded BN bias, residual, ReLU) as Winograd F(4x4, 3x3) on the gfx950 fp32 matrix
// cores (cerb_net_set_conv_algo(5)).  36 products per 4x4 output pixels and input channel instead of 64 for F(2x2) (144 direct): 1.78x
// fewer matrix instructions than conv_wino.hip AND 1.78x less input-transform volume per output pixel (a 6x6 patch per 16 outputs
// instead of a 4x4 patch per 4) -- the input path is what bounded the three F(2x2) kernels.  Products are exact fp32
// FMAs; the transforms (points 0, +-1, +-2, inf) move the probability maps by < 4e-6 against an fp64 evaluation of the network
// (tests/tools/dev_wino4_numerics.py), 1.5x the direct fp32 convolution's own distance.
//
//   Y = A^T [ sum_cin (G g G^T) .* (B^T d B) ] A        d 6x6 input patch, g 3x3 filter (BN folded), Y 4x4 outputs
//
// Work decomposition (conv_wino16d.hip's, grown to 36 positions):
//   * item = two 16x16-pixel blocks (2 x 16 tiles of 4x4 outputs) x 64 output channels; persistent workgroups of 4 waves, ONE per CU;
//   * a wave owns ALL 36 positions of 16 output channels for the 32 tiles on v_mfma_f32_16x16x4_f32: 36 x 2 x 4 = 288 accumulator
//     registers -- one wave per SIMD, accumulators in the AccVGPR half of the 512-register file -- so every weight register feeds two
//     matrix instructions (a 16-tile item would need 1 KiB of weights per wave per 128 cycles = the L2's whole bandwidth) and the
//     output transform A^T M A is additions in registers: no exchange through LDS;
//   * 16-channel chunks, V tile [36][32 tiles][16 ch] = 72 KiB, double-buffered (144 of the CU's 160 KiB): one barrier per chunk;
//     16-byte slots of a tile's channel vector are XOR-swizzled by the tile index so that ds_read_b128 of 16 tiles x 4 k-slots and the
//     8-byte transform writes are bank-conflict-free without padding;
//   * thread = (tile, channel pair): the raw 6x6 patch is 36 float2 loaded straight from global memory (uniform offsets ride in the
//     buffer instruction's scalar offset), transformed in place one 1-D pass per step in the shadow of the matrix pipe.
// Reference layers: models/utils/conv_layers.py:24-60 (_ConvLayer) and models/backbone/resnet.py:81-97 (BasicBlock).
#include <type_traits>

#include "wino_common.h"

namespace {
constexpr int NPOS = 36;
constexpr int NT = 32;                        // tiles per item: two blocks of 4x4 tiles
constexpr int CB = 16;                        // input channels per LDS pass
constexpr int V_FLOATS = NPOS * NT * CB;      // one V buffer: 72 KiB
constexpr int LDS_BYTES = 2 * V_FLOATS * 4;   // double-buffered: 144 KiB
static_assert(256 * OPX + 16 <= V_FLOATS, "a block's outputs are staged in one V buffer");
#ifdef W4_PROF
constexpr int PROF_BYTES = 16 * 40 * 8;
#else
constexpr int PROF_BYTES = 0;
#endif
constexpr int NS = NPOS;                      // steps per chunk: one position each (one 16-byte weight load, two ds_read_b128, 8 MFMAs)
#ifndef W4_RING
#define W4_RING 12
#endif
constexpr int RING = W4_RING;                 // weight operand slots (NS % RING == 0: the slot of a step does not depend on the chunk)
#ifndef W4_PRE
#define W4_PRE 8
#endif
constexpr int PRE = W4_PRE;                   // steps of the NEXT item whose weights are requested before an item's output stores
#ifndef W4_WD
#define W4_WD 8
#endif
constexpr int WD = W4_WD;                     // weight prefetch distance in steps
#ifndef W4_WB
#define W4_WB 4
#endif
constexpr int WB = W4_WB;                     // weight burst size in steps
#ifndef W4_PL
#define W4_PL 3
#endif
constexpr int PL = W4_PL;                     // patch loads issued per step
#ifndef W4_P0
#define W4_P0 0
#endif
constexpr int P0 = W4_P0;                     // first step that issues patch loads
#ifndef W4_TQ
#define W4_TQ 18
#endif
#ifndef W4_PATCH_AUX
#define W4_PATCH_AUX 0
#endif
#ifndef W4_STORE_AUX
#define W4_STORE_AUX 0
#endif
constexpr int TQ = W4_TQ;                     // the next chunk's patch is masked at TQ, transformed at TQ+1 .. TQ+12, written at TQ+7 .. TQ+12
static_assert(NS % RING == 0 && WD + WB <= RING && NS % WB == 0 && PRE >= WD && PRE <= RING, "weight ring");
#ifdef W4_ABL_HALFPATCH
static_assert(P0 + (W4_ABL_HALFPATCH + PL - 1) / PL <= TQ && TQ + 13 < NS, "ablation: the loads that are issued must precede the transform");
#else
static_assert(P0 + (36 + PL - 1) / PL <= TQ && TQ + 13 < NS, "the patch must be requested before its transform starts");
#endif
constexpr int BIAS_XI = 7;                    // A^T[i][1] A[1][j] = 1 for all 16 outputs: the bias enters through position (1, 1)
constexpr int CHUNK_W_BYTES = NPOS * 4 * 1024;  // packed weights of one (cout block, 16-channel chunk): 144 KiB
constexpr int WAVE_W_BYTES = NPOS * 1024;       // one wave's share: 36 steps x 1 KiB

#ifdef W4_PROF
// developer instrumentation (scripts/dev_w4prof.py): wave 0 of workgroup W4_PROF stamps s_memtime at every step of its second item
__device__ unsigned long long w4_prof_buf[16 * 40];
#endif

struct Blk {
    int n, by, bx;  // image, block row / column inside the launch's block grid
};
struct Item {
    int g, cb;
    Blk b0, b1;  // (no array: a dynamically indexed member would keep the whole struct in scratch, i.e. in vector registers)
    int nvalid;  // 2, or 1 when the launch has an odd number of blocks and this is the last pair (block 1 repeats block 0, stores dropped)
};
}  // namespace

// STATS 1 (training forward): the output stage also leaves BatchNorm statistics partials per block (ConvParams::bn_part) -- a separate
// instantiation, so that the inference kernels are the same code as without it.
// STATS 2 (training backward, this launch is a data gradient whose output is the gradient dz behind a BatchNorm + ReLU and its only writer): the output stage
// reads the BatchNorm's INPUT y at its own pixels and leaves that BatchNorm's backward sums per block -- (sum dz', sum dz' xhat), dz' = dz where bn_out(y) > 0 --
// in the same place and layout: the BatchNorm's reduction pass over dz and y (train_kernels.hip: bn_bwd_partial_kernel) does not run (ConvParams::bst_*).
template <bool HAS_RES, int STATS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void conv_wino4_kernel(ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ __attribute__((aligned(16))) float bnred[STATS ? 4 * 16 * 8 * 2 : 4];  // STATS: [wave][channel quad][4 sums, 4 sums of squares], doubles for STATS 1 (wino4_store_block)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int a = __builtin_amdgcn_readfirstlane(tid >> 6);  // this wave's 16 output channels of the item's 64; input path: block a >> 1
    const int m = lane & 15;                                 // MFMA row (cout) / column (tile within a block)
    const int ks = lane >> 4;                                // k-slot

    const int ncb = p.Cout >> 6;
    const int nblk = p.N * p.tiles_y * p.tiles_x;  // blocks per group
    const int npair = (nblk + 1) >> 1;
    const int per_group = npair * ncb;
    const int total = per_group * p.groups;
    const int nchunk = p.Cin / CB;
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int base_cnt = total / (int)gridDim.x, rem_cnt = total % (int)gridDim.x;
    int item = lb * base_cnt + min(lb, rem_cnt);
#ifndef W4_CONTIGUOUS  // workgroup lb takes items lb, lb + G, ...: neighbouring blocks (shared halo lines, the cout blocks of one patch) run at the
                       // same time on one XCD and meet in its L2 (-1 % / -3 % against contiguous item ranges per workgroup)
    const int ISTEP = (int)gridDim.x;
    item = lb;
    const int item_end = total;
#else
    const int ISTEP = 1;
    const int item_end = item + base_cnt + (lb < rem_cnt ? 1 : 0);
#endif
    if (item >= item_end) return;
#ifdef W4_PROF
    const int prof_item = item + ISTEP;
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
    auto oy0 = [&](const Blk& b) { return (b.by + p.ty_off) * BLK; };
    auto ox0 = [&](const Blk& b) { return (b.bx + p.tx_off) * BLK; };
    auto in_base = [&](int g, const Blk& b) {
        return reinterpret_cast<const char*>(p.in + g * p.in_gs) + ((((long long)b.n * p.H + (oy0(b) - 1)) * p.W + (ox0(b) - 1)) * p.Cin) * 4;
    };
    auto w_base = [&](const Item& w) {
        return reinterpret_cast<const char*>(p.wpack + w.g * p.w_gs) + (long long)w.cb * nchunk * CHUNK_W_BYTES + a * WAVE_W_BYTES;
    };
    auto hangs_over = [&](const Blk& b) { return oy0(b) + BLK > p.H || ox0(b) + BLK > p.W; };
    auto edge_bits = [&](const Blk& b) {  // 1 top, 2 bottom, 4 left, 8 right
        return (oy0(b) == 0 ? 1 : 0) | (oy0(b) + BLK == p.H ? 2 : 0) | (ox0(b) == 0 ? 4 : 0) | (ox0(b) + BLK == p.W ? 8 : 0);
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
    const unsigned ioff = (unsigned)((((4 * tty) * p.W + 4 * ttx) * p.Cin + 2 * c) * 4);
    const int vw = t * CB + (((c >> 1) ^ ((tm & 8) ? 3 : 0)) << 2) + 2 * (c & 1);  // V write position (floats); position xi adds xi*NT*CB
    const int vr = m * CB + ((ks ^ ((m & 8) ? 3 : 0)) << 2);                       // V read position, block 0; block 1 adds 16*CB
    const unsigned wlane = (unsigned)lane * 16u;
    const int rowb = p.W * p.Cin * 4, pixb = p.Cin * 4;

    f32x2 d[6][6];  // raw patch of the NEXT chunk (two channels), transformed in place in the shadow of the matrix pipe
    const bool lane_top = (tty == 0), lane_bot = (tty == 3), lane_left = (ttx == 0), lane_right = (ttx == 3);
    // zero padding at the image border by ADDRESS (conv_wino4b.hip): nine lane offsets per chunk instead of ~100 VALU instructions of masking
    struct EdgeOff { unsigned o[3][3]; };
    auto edge_offsets = [&](int bits) __attribute__((always_inline)) {
        EdgeOff e;
        const bool zt = (bits & 1) && lane_top, zb = (bits & 2) && lane_bot, zl = (bits & 4) && lane_left, zr = (bits & 8) && lane_right;
        const unsigned col[3] = {zl ? 0x80000000u : ioff, ioff, zr ? 0x80000000u : ioff};
#pragma unroll
        for (int qc = 0; qc < 3; ++qc) {
            e.o[0][qc] = zt ? 0x80000000u : col[qc];
            e.o[1][qc] = col[qc];
            e.o[2][qc] = zb ? 0x80000000u : col[qc];
        }
#pragma unroll
        for (int rc = 0; rc < 3; ++rc)
#pragma unroll
            for (int qc = 0; qc < 3; ++qc) asm volatile("" : "+v"(e.o[rc][qc]));
        return e;
    };
    auto issue = [&](__amdgpu_buffer_rsrc_t r, const EdgeOff& e, int chunk_off, int k) __attribute__((always_inline)) {
        const int rr = k / 6, qq = k % 6;
        d[rr][qq] = buf_load2<W4_PATCH_AUX>(r, e.o[rr == 0 ? 0 : rr == 5 ? 2 : 1][qq == 0 ? 0 : qq == 5 ? 2 : 1], chunk_off + rr * rowb + qq * pixb);
    };
    auto mask_border = [&](const Blk& b) __attribute__((always_inline)) {
        const f32x2 z = {0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const int gy = oy0(b) - 1 + 4 * tty + r, gx = ox0(b) - 1 + 4 * ttx + q;
                const bool ok = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
                d[r][q] = ok ? d[r][q] : z;
            }
    };
    // B^T x, in place (wino_common.h: wino4_bt6), with its constants pinned in registers
    f32x2 k2 = {2.f, 2.f}, k4 = {4.f, 4.f}, k5 = {5.f, 5.f};
    asm volatile("" : "+v"(k2), "+v"(k4), "+v"(k5));
    auto pass_v = [&](int q) { wino4_bt6(d[0][q], d[1][q], d[2][q], d[3][q], d[4][q], d[5][q], k2, k4, k5); };  // down column q
    auto pass_h = [&](int r) { wino4_bt6(d[r][0], d[r][1], d[r][2], d[r][3], d[r][4], d[r][5], k2, k4, k5); };  // along row r
    auto write_row = [&](int buf, int r) {
#pragma unroll
        for (int b = 0; b < 6; ++b) *reinterpret_cast<f32x2*>(lds + buf * V_FLOATS + (r * 6 + b) * NT * CB + vw) = d[r][b];
    };

    // ---- prologue ------------------------------------------------------------------------------------------------------------
    Item w = decode(item);
    {
        const Blk b0_ = mine(w);
        const __amdgpu_buffer_rsrc_t r0 = make_rsrc_lim(in_base(w.g, b0_));
        const EdgeOff e0 = edge_offsets(hangs_over(b0_) ? 0 : edge_bits(b0_));
#pragma unroll
        for (int k = 0; k < 36; ++k) issue(r0, e0, 0, k);
        if (hangs_over(b0_)) mask_border(b0_);
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) pass_v(q);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        pass_h(r);
        write_row(0, r);
    }
    int vbuf = 0;  // the buffer the CURRENT chunk reads; the next chunk's patch goes to vbuf ^ 1
    __syncthreads();
    __amdgpu_buffer_rsrc_t rw = make_rsrc(w_base(w));
    // Weight stream in bursts (conv_wino16d.hip): every WB steps the operands of steps q + WD .. q + WD + WB - 1 are requested at once; the
    // operand of step q lives in slot q % RING.  Steps past the chunk's 36 belong to the next chunk, or to the next item's first chunk.
    f32x4 wq[RING];
#pragma unroll
    for (int dd = 0; dd < PRE; ++dd) wq[dd] = buf_load(rw, wlane, dd * 1024);
    f32x4 bnext;
    auto load_bias = [&](const Item& wi) {
        const float* bias = p.bias + wi.g * p.bias_gs + wi.cb * 64 + 16 * a;
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bias), 0, 64, 0x00020000);
        bnext = buf_load(rb, (unsigned)ks * 16u, 0);
    };
    load_bias(w);

    for (;;) {
        f32x4 acc[NPOS][2];
        const bool more_items = item + ISTEP < item_end;
        const Item wnx = more_items ? decode(item + ISTEP) : w;
        const __amdgpu_buffer_rsrc_t rw_nx = more_items ? make_rsrc(w_base(wnx)) : rw;
        const Blk bcur = mine(w), bnx = mine(wnx);
        const bool mask_cur = hangs_over(bcur), mask_next = hangs_over(bnx);
        const int edge_next = edge_bits(bnx), edge_cur = edge_bits(bcur);
        const char* in_cur = in_base(w.g, bcur);
        const char* in_nx = in_base(wnx.g, bnx);
        acc[BIAS_XI][0] = bnext;
        acc[BIAS_XI][1] = bnext;
#ifdef W4_PROF
        const bool prof_on = (blockIdx.x == W4_PROF) && a == 0 && (item == prof_item);
#define W4_STAMP(k) do { if (prof_on && lane == 0) reinterpret_cast<unsigned long long*>(lds + 2 * V_FLOATS)[15 * 40 + (k)] = __builtin_readcyclecounter(); } while (0)
#else
#define W4_STAMP(k) do { } while (0)
#endif

        auto chunk = [&](auto first_tag, int ch) __attribute__((always_inline)) {
            constexpr bool FIRST = decltype(first_tag)::value;
            const bool last_ch = (ch == nchunk - 1);
            const Blk bp_ = last_ch ? bnx : bcur;
            const bool mask_nx = last_ch ? mask_next : mask_cur;
            const int edge_nx = last_ch ? edge_next : edge_cur;
#ifdef W4_ABL_PATCHHOT
            const __amdgpu_buffer_rsrc_t r_stage = make_rsrc_lim(reinterpret_cast<const char*>(p.in) + (blockIdx.x & 7) * 65536);  // cache-resident
            const int stage_off = 0;
#else
            const __amdgpu_buffer_rsrc_t r_stage = make_rsrc_lim(last_ch ? in_nx : in_cur);
            const int stage_off = (last_ch ? 0 : ch + 1) * (CB * 4);
#endif
            const EdgeOff eN = edge_offsets(mask_nx ? 0 : edge_nx);
            const int wcur_off = ch * CHUNK_W_BYTES;
            const __amdgpu_buffer_rsrc_t rw_over = last_ch ? rw_nx : rw;
            const int wover_off = last_ch ? 0 : (ch + 1) * CHUNK_W_BYTES;
            const float* vsrc = lds + vbuf * V_FLOATS + vr;
            const int wbuf = vbuf ^ 1;

            f32x4 bb[2][2];  // B operands (blocks 0, 1) of step q in bb[q & 1]
            bb[0][0] = *reinterpret_cast<const f32x4*>(vsrc);
            bb[0][1] = *reinterpret_cast<const f32x4*>(vsrc + 16 * CB);
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const int xi = q;
#ifdef W4_PROF
                if (prof_on && ch < 16 && lane == 0) reinterpret_cast<unsigned long long*>(lds + 2 * V_FLOATS)[ch * 40 + q] = __builtin_readcyclecounter();
#endif
#ifndef W4_ABL_NOWLOAD
                if (q % WB == 0) {
#pragma unroll
                    for (int dd = q + WD; dd < q + WD + WB; ++dd) {
                        if (FIRST && dd < PRE) continue;  // requested before the previous item's stores (or in the prologue)
                        if (dd < NS) wq[dd % RING] = buf_load(rw, wlane, wcur_off + dd * 1024);
                        else wq[(dd - NS) % RING] = buf_load(rw_over, wlane, wover_off + (dd - NS) * 1024);
                    }
                }
#endif
                if (q + 1 < NS) {
                    bb[(q + 1) & 1][0] = *reinterpret_cast<const f32x4*>(vsrc + (q + 1) * NT * CB);
                    bb[(q + 1) & 1][1] = *reinterpret_cast<const f32x4*>(vsrc + (q + 1) * NT * CB + 16 * CB);
                }
#ifndef W4_ABL_NOPATCH
                if (q >= P0 && (q - P0) * PL < 36 && q <= TQ) {  // next chunk's patch: PL loads per step
#pragma unroll
                    for (int u = 0; u < PL; ++u)
#ifdef W4_ABL_HALFPATCH
                        if ((q - P0) * PL + u < W4_ABL_HALFPATCH) issue(r_stage, eN, stage_off, (q - P0) * PL + u);
#else
                        if ((q - P0) * PL + u < 36) issue(r_stage, eN, stage_off, (q - P0) * PL + u);
#endif
                }
#endif
                // the next chunk's patch landed: mask, B^T d B (one 1-D pass per step) and the V writes into the OTHER buffer
                if (q == TQ) {
                    if (mask_nx) mask_border(bp_);
                }
#ifndef W4_ABL_NOXF
                if (q > TQ && q <= TQ + 6) pass_v(q - TQ - 1);
                if (q > TQ + 6 && q <= TQ + 12) pass_h(q - TQ - 7);
#endif
#ifndef W4_ABL_NOVWRITE
                if (q > TQ + 6 && q <= TQ + 12) write_row(wbuf, q - TQ - 7);
#endif
                __builtin_amdgcn_sched_barrier(0);
                const f32x4 av = wq[q % RING];
                const f32x4 b0 = bb[q & 1][0], b1 = bb[q & 1][1];
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    if (FIRST && tt == 0 && xi != BIAS_XI) {
                        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                        acc[xi][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tt], b0[tt], z, 0, 0, 0);
                        acc[xi][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tt], b1[tt], z, 0, 0, 0);
                    } else {
                        acc[xi][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tt], b0[tt], acc[xi][0], 0, 0, 0);
                        acc[xi][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tt], b1[tt], acc[xi][1], 0, 0, 0);
                    }
                }
            }
#ifndef W4_ABL_NOBAR
            __syncthreads();  // everybody has read this chunk's V and written the next one's
#endif
            vbuf ^= 1;
        };
        chunk(std::true_type{}, 0);
        for (int ch = 1; ch < nchunk; ++ch) chunk(std::false_type{}, ch);

        // ---- output transform A^T M A, entirely in registers; lane (m, ks): tile m of each block, channels 4 ks .. + 3 of the wave's 16 -------
        // vmcnt retires in order across loads AND stores, and the stores' acknowledgements take microseconds: everything the next item
        // needs during its first PRE steps is requested here, before this item's stores enter the queue (its steps 0 .. WD-1 went out
        // during the last chunk).  The raw-patch registers are dead at this point, so the extra slots cost nothing in the steady state.
        W4_STAMP(0);
#pragma unroll
        for (int dd = WD; dd < PRE; ++dd) wq[dd % RING] = buf_load(rw_nx, wlane, dd * 1024);
        load_bias(wnx);
        {
            int lane_o = lane;
            asm volatile("" : "+v"(lane_o));  // recomputed per item: keeps what derives from it out of the MFMA phase's register budget
            float* stg = lds + (vbuf ^ 1) * V_FLOATS;  // the V buffer the last chunk has finished with; the next item's second chunk rewrites it
#pragma unroll
            for (int tb = 0; tb < 2; ++tb) {
                const Blk bo = tb ? w.b1 : w.b0;
                W4_STAMP(1 + 3 * tb);
                wino4_store_block<HAS_RES, STATS, false, 0, W4_STORE_AUX>(
                    p, stg, bnred, a, lane_o, Wino4Block{w.g, w.cb, bo.n, bo.by, bo.bx}, tb == 1 && w.nvalid == 1,
                    [&](int xi) __attribute__((always_inline)) -> const f32x4& { return acc[xi][tb]; }, [](int, int&, int&, int&) {},
                    [&](int k) __attribute__((always_inline)) { if (k == 0) W4_STAMP(2 + 3 * tb); });
            }
        }
#ifdef W4_PROF
        W4_STAMP(7);
        if (prof_on) {
            __builtin_amdgcn_s_waitcnt(0);
            W4_STAMP(8);
            if (lane == 0) reinterpret_cast<unsigned long long*>(lds + 2 * V_FLOATS)[(nchunk < 16 ? nchunk : 15) * 40 + 39] = __builtin_readcyclecounter();
            __builtin_amdgcn_s_waitcnt(0);
            for (int i = lane; i < 16 * 40; i += 64) w4_prof_buf[i] = reinterpret_cast<unsigned long long*>(lds + 2 * V_FLOATS)[i];
        }
#endif
        if (!more_items) break;
        item += ISTEP;
        w = wnx;
        rw = rw_nx;
    }
}

template <bool HAS_RES>
static hipError_t launch_wino4(ConvParams p, hipStream_t st) {
    const long long nblk = wino4_block_grid(p);
    const long long items = (long long)p.groups * ((nblk + 1) / 2) * (p.Cout / 64);
    const int stats = wino4_stats(p);
    if (stats && HAS_RES) return hipErrorInvalidValue;
    p.bn_bpg = (int)nblk;
    auto kern = stats == 2 ? conv_wino4_kernel<false, 2> : stats == 1 ? conv_wino4_kernel<false, 1> : conv_wino4_kernel<HAS_RES, 0>;
    static bool attr_done[3][64] = {};
    return wino4_launch(kern, attr_done[stats], items, LDS_BYTES + PROF_BYTES, p, st);
}

#ifdef W4_PROF
extern "C" int cerb_w4_prof_read(unsigned long long* dst) { return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(w4_prof_buf), sizeof(unsigned long long) * 16 * 40); }
#endif

hipError_t cerb_launch_wino4(ConvParams p, hipStream_t st) {
    if (p.Cin % CB || p.Cout % 64) return hipErrorInvalidValue;
    return p.resid ? launch_wino4<true>(p, st) : launch_wino4<false>(p, st);
}
