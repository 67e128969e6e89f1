// Instance metrics on the device: the sparse contingency table between two int32 label maps and the counters of PQ / AJI / Dice2 / Dice1 derived
// from it (include/cerberus_hip.h: cerb_inst_areas, cerb_inst_pairs, cerb_inst_pairs_compact, cerb_inst_pair_stats; cerberus_amd/inst_metrics.py).
//
// Both pixel passes walk the map in 64 x 64 tiles, one workgroup (256 threads) per tile.  A thread owns four consecutive pixels of a row (one 16-byte
// load per map where base and row stride allow it), a wave a 64 x 4 patch: instances are compact, so most lanes of a wave hold the same id.
//   area pass  runs of equal ids are merged in registers, equal ids are summed over the wave (a few leader rounds), the leader issues ONE 64-bit
//              atomic per (wave, id); lanes still pending after IM_ROUNDS rounds (a noise map) add on their own.
//   pair pass  the same with the 64-bit key (true index << 32 | pred index) into an LDS open-addressing table of IM_LDS slots; the tile's entries are
//              flushed once into the global open-addressing table (key by 64-bit compare-and-swap, count by a 64-bit add).  A key that finds no LDS
//              slot within IM_LDS_PROBES probes goes straight to the global table.  Global probing is bounded by IM_G_PROBES: past it the update is
//              DROPPED and the overflow word is set -- the caller reads {n_pairs, overflow} and runs the pass again on a larger table.  Slots are
//              always taken modulo the (power-of-two) capacity: an overflow never loops and never leaves the table.
// Ids outside [1, n_ids] count as background and never index a table.  Every pixel offset is a long long (y * row_stride + x); nothing outside h x w is
// read.  All counts are integers: the tables do not depend on arrival order.  The reduction (pair_stats) takes every decision -- match 2c > u, the AJI
// arg-max by cross-multiplication in 128 bits, ties to the smaller pred id -- in integers, and sums the matched IoUs in float64 in ONE fixed order
// (per-true-instance values stored, then a single workgroup adds them by a fixed stride and a fixed tree), so two runs agree bitwise.
#include "cerb_net.h"

namespace {

constexpr int IM_BLOCK = 256;
constexpr int IM_TILE = 64;            // tile side in pixels; a block pass covers 64 x 16, four passes a tile
constexpr int IM_ROUNDS = 6;           // leader rounds of the wave aggregation
constexpr int IM_LDS = 1024;           // LDS table slots (8-byte key + 4-byte count)
constexpr int IM_LDS_PROBES = 16;
constexpr int IM_G_PROBES = 128;
constexpr int IM_META = 4;             // {n_pairs, overflow, table updates kept in LDS, updates sent to the global table}
typedef unsigned long long u64;

__device__ __forceinline__ u64 im_hash(u64 k) {  // 64-bit finaliser (splitmix64)
    k ^= k >> 30, k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27, k *= 0x94d049bb133111ebull;
    return k ^ (k >> 31);
}
__device__ __forceinline__ unsigned im_wave_sum(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ long long im_wave_sum64(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ u64 im_shfl64(u64 v, int lane) {
    const unsigned lo = __shfl((unsigned)v, lane, 64), hi = __shfl((unsigned)(v >> 32), lane, 64);
    return ((u64)hi << 32) | lo;
}

// four pixels of row y starting at column x (x % 4 == 0): 0 outside the map
template <bool VEC>
__device__ __forceinline__ void im_load4(const int* __restrict__ base, long long row_stride, int y, int x, int h, int w, int v[4]) {
    v[0] = v[1] = v[2] = v[3] = 0;
    if (y >= h || x >= w) return;
    const long long off = (long long)y * row_stride + x;
    if (VEC && x + 3 < w) {
        const int4 q = *reinterpret_cast<const int4*>(base + off);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i < w) v[i] = base[off + i];
    }
}
// ids outside [1, n_ids] -> 0 (unsigned arithmetic: no overflow for INT_MIN; n_ids <= IM_MAX_IDS keeps 0x80000000 - 1 out)
constexpr int IM_MAX_IDS = 0x7ffffffe;
__device__ __forceinline__ int im_clean(int id, int n_ids) { return ((unsigned)id - 1u < (unsigned)n_ids) ? id : 0; }

// ---- area pass -----------------------------------------------------------------------------------------------------------------------------
// every lane of the wave calls this together; id 0 = nothing to add
__device__ __forceinline__ void im_area_add(u64* __restrict__ area, int id, unsigned cnt, int lane) {
    for (int r = 0; r < IM_ROUNDS; ++r) {
        const u64 pend = __ballot(id != 0);
        if (pend == 0) return;
        const int leader = __ffsll((long long)pend) - 1;
        const int lid = __shfl(id, leader, 64);
        const bool mine = id == lid;
        const unsigned s = im_wave_sum(mine ? cnt : 0u);
        if (lane == leader) atomicAdd(area + lid, (u64)s);
        if (mine) id = 0;
    }
    if (id != 0) atomicAdd(area + id, (u64)cnt);
}

template <bool VEC>
__global__ __launch_bounds__(IM_BLOCK) void im_area_kernel(const int* __restrict__ lab, long long row_stride, int h, int w, int n_ids,
                                                           long long tiles_x, long long n_tiles, u64* __restrict__ area) {
    const int lane = threadIdx.x & 63, r = threadIdx.x >> 4, q = threadIdx.x & 15;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int y0 = (int)(tile / tiles_x) * IM_TILE, x = (int)(tile % tiles_x) * IM_TILE + q * 4;
        for (int pass = 0; pass < IM_TILE / 16; ++pass) {
            int v[4];
            im_load4<VEC>(lab, row_stride, y0 + pass * 16 + r, x, h, w, v);
            int id[4];
            unsigned cnt[4] = {0, 0, 0, 0};
            int n = 0;
            id[0] = id[1] = id[2] = id[3] = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = im_clean(v[i], n_ids);
                if (i > 0 && c == id[n]) {
                    cnt[n] += 1;
                } else {
                    if (i > 0 && id[n] != 0) ++n;
                    id[n] = c, cnt[n] = 1;
                }
            }
            // runs of background hold id 0 and are skipped; slots past the last run are 0 too
#pragma unroll
            for (int i = 0; i < 4; ++i) im_area_add(area, i <= n ? id[i] : 0, cnt[i], lane);
        }
    }
}

// ---- pair pass -----------------------------------------------------------------------------------------------------------------------------
struct ImTable {
    u64* keys;    // [cap], 0 = empty (a key holds two indices >= 1 and is never 0)
    u64* counts;  // [cap]
    u64 mask;     // cap - 1, cap a power of two
    u64* meta;    // IM_META words
};

// bounded probing; drops the update and raises the overflow word when no slot is found.  Returns 1 when this call took a free slot (a new pair): the
// caller counts those in a register -- one counter word updated per new pair would serialise the whole pass on that word.
__device__ __forceinline__ unsigned im_global_add(const ImTable& t, u64 key, u64 cnt) {
    u64 s = im_hash(key) & t.mask;
    for (int probe = 0; probe < IM_G_PROBES; ++probe) {
        u64 prev = t.keys[s];
        if (prev == 0) prev = atomicCAS(t.keys + s, 0ull, key);
        if (prev == 0 || prev == key) {
            atomicAdd(t.counts + s, cnt);
            return prev == 0 ? 1u : 0u;
        }
        s = (s + 1) & t.mask;
    }
    atomicMax(t.meta + 1, 1ull);
    return 0u;
}

// true when the update was kept in LDS
__device__ __forceinline__ bool im_lds_add(u64* lkeys, unsigned* lcnt, u64 key, unsigned cnt) {
    unsigned s = (unsigned)im_hash(key) & (IM_LDS - 1);
    for (int probe = 0; probe < IM_LDS_PROBES; ++probe) {
        u64 prev = lkeys[s];
        if (prev == 0) prev = atomicCAS(lkeys + s, 0ull, key);
        if (prev == 0 || prev == key) {
            atomicAdd(lcnt + s, cnt);
            return true;
        }
        s = (s + 1) & (IM_LDS - 1);
    }
    return false;
}

template <bool VEC>
__global__ __launch_bounds__(IM_BLOCK) void im_pair_kernel(const int* __restrict__ tru, long long t_stride, const int* __restrict__ prd, long long p_stride,
                                                           int h, int w, const int* __restrict__ t_index, int n_t_ids, const int* __restrict__ p_index,
                                                           int n_p_ids, long long tiles_x, long long n_tiles, ImTable tab) {
    __shared__ u64 lkeys[IM_LDS];
    __shared__ unsigned lcnt[IM_LDS];
    const int lane = threadIdx.x & 63, r = threadIdx.x >> 4, q = threadIdx.x & 15;
    unsigned n_lds = 0, n_glob = 0, n_new = 0;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        for (int i = threadIdx.x; i < IM_LDS; i += IM_BLOCK) lkeys[i] = 0, lcnt[i] = 0;
        __syncthreads();
        const int y0 = (int)(tile / tiles_x) * IM_TILE, x = (int)(tile % tiles_x) * IM_TILE + q * 4;
        for (int pass = 0; pass < IM_TILE / 16; ++pass) {
            int tv[4], pv[4];
            im_load4<VEC>(tru, t_stride, y0 + pass * 16 + r, x, h, w, tv);
            im_load4<VEC>(prd, p_stride, y0 + pass * 16 + r, x, h, w, pv);
            u64 key[4] = {0, 0, 0, 0};
            unsigned cnt[4] = {0, 0, 0, 0};
            int n = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = im_clean(tv[i], n_t_ids), p = im_clean(pv[i], n_p_ids);
                // the index tables hold 0 for ids that do not occur; both sides are read only for ids inside their bounds
                const unsigned ti = t ? (unsigned)t_index[t] : 0u, pi = p ? (unsigned)p_index[p] : 0u;
                const u64 k = (ti && pi) ? (((u64)ti << 32) | pi) : 0ull;
                if (i > 0 && k == key[n]) {
                    cnt[n] += 1;
                } else {
                    if (i > 0 && key[n] != 0) ++n;
                    key[n] = k, cnt[n] = 1;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                u64 k = i <= n ? key[i] : 0ull;
                unsigned c = cnt[i];
                // equal keys of the wave are summed onto a leader lane first; what is still pending after the rounds goes to LDS as it is
                for (int round = 0; round < IM_ROUNDS; ++round) {
                    const u64 pend = __ballot(k != 0);
                    if (pend == 0) break;
                    const int leader = __ffsll((long long)pend) - 1;
                    const u64 lk = im_shfl64(k, leader);
                    const bool mine = k == lk;
                    const unsigned s = im_wave_sum(mine ? c : 0u);
                    if (lane == leader) {
                        if (im_lds_add(lkeys, lcnt, lk, s)) ++n_lds;
                        else n_new += im_global_add(tab, lk, s), ++n_glob;
                    }
                    if (mine) k = 0;
                }
                if (k != 0) {
                    if (im_lds_add(lkeys, lcnt, k, c)) ++n_lds;
                    else n_new += im_global_add(tab, k, c), ++n_glob;
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < IM_LDS; i += IM_BLOCK)
            if (lkeys[i] != 0) n_new += im_global_add(tab, lkeys[i], lcnt[i]), ++n_glob;
        __syncthreads();
    }
    // the block's three counters: wave sums, then one update per counter and block (the grid is a few blocks per CU, see cerb_inst_pairs)
    const unsigned a = im_wave_sum(n_new), b = im_wave_sum(n_lds), c = im_wave_sum(n_glob);
    if (lane == 0) lcnt[3 * (threadIdx.x >> 6)] = a, lcnt[3 * (threadIdx.x >> 6) + 1] = b, lcnt[3 * (threadIdx.x >> 6) + 2] = c;
    __syncthreads();
    if (threadIdx.x < 3) {
        u64 v = 0;
        for (int wv = 0; wv < IM_BLOCK / 64; ++wv) v += lcnt[3 * wv + threadIdx.x];
        if (v) atomicAdd(tab.meta + (threadIdx.x == 0 ? 0 : threadIdx.x + 1), v);
    }
}

__global__ void im_compact_kernel(const u64* __restrict__ keys, const u64* __restrict__ counts, long long cap, long long* __restrict__ keys_out,
                                  long long* __restrict__ counts_out, long long max_out, u64* __restrict__ n_out) {
    const int lane = threadIdx.x & 63;
    for (long long s0 = blockIdx.x * (long long)blockDim.x; s0 < cap; s0 += (long long)gridDim.x * blockDim.x) {  // (uniform over the block)
        const long long s = s0 + threadIdx.x;
        const u64 k = s < cap ? keys[s] : 0ull;
        const u64 occ = __ballot(k != 0);  // one counter update per wave: the leader reserves a run of output slots
        if (occ == 0) continue;
        const int leader = __ffsll((long long)occ) - 1;
        u64 base = 0;
        if (lane == leader) base = atomicAdd(n_out, (u64)__popcll(occ));
        base = im_shfl64(base, leader);
        const u64 at = base + (u64)__popcll(occ & ((1ull << lane) - 1ull));
        if (k != 0 && at < (u64)max_out) keys_out[at] = (long long)k, counts_out[at] = (long long)counts[s];
    }
}

// ---- reduction over the sorted pairs -----------------------------------------------------------------------------------------------------------
struct ImStats {
    const long long* keys;    // sorted ascending
    const long long* counts;
    long long n_pairs;
    const long long* t_area;  // [n_t], index - 1
    const long long* p_area;  // [n_p]
    const int* t_type;        // [n_t] or nullptr
    const int* p_type;        // [n_p] or nullptr
    int n_t, n_p, cls;
    long long* summary;       // CERB_INST_SUMMARY_WORDS
    double* sum_iou;
    double* iou;              // [n_t] workspace
    unsigned char* used;      // [n_p] workspace
};
enum { S_TP, S_FP, S_FN, S_AJI_I, S_AJI_U, S_D2_I, S_D2_T, S_D1_I, S_D1_T, S_NT, S_NP, S_WORDS };
static_assert(S_WORDS <= CERB_INST_SUMMARY_WORDS, "summary layout");

// a * b > c * d in 128 bits
__device__ __forceinline__ bool im_mul_gt(u64 a, u64 b, u64 c, u64 d) {
    const u64 h1 = __umul64hi(a, b), l1 = a * b, h2 = __umul64hi(c, d), l2 = c * d;
    return h1 > h2 || (h1 == h2 && l1 > l2);
}

__device__ __forceinline__ void im_flush(long long* acc, const long long* v, int n, int lane) {
    for (int i = 0; i < n; ++i) {
        const long long s = im_wave_sum64(v[i]);
        if (lane == 0 && s != 0) atomicAdd((u64*)acc + i, (u64)s);
    }
}

__global__ __launch_bounds__(IM_BLOCK) void im_stats_true_kernel(ImStats a) {
    long long v[S_WORDS];
    for (int i = 0; i < S_WORDS; ++i) v[i] = 0;
    for (long long i0 = blockIdx.x * (long long)IM_BLOCK; i0 < a.n_t; i0 += (long long)gridDim.x * IM_BLOCK) {
        const long long ti = i0 + threadIdx.x + 1;  // 1-based true index
        if (ti > a.n_t) continue;
        double iou = 0.0;
        if (a.cls < 0 || a.t_type == nullptr || a.t_type[ti - 1] == a.cls) {
            const u64 at = (u64)a.t_area[ti - 1];
            v[S_NT] += 1, v[S_D1_T] += (long long)at;
            long long lo = 0, hi = a.n_pairs;  // first pair of this true index
            const long long first = ti << 32;
            while (lo < hi) {
                const long long mid = lo + (hi - lo) / 2;
                if (a.keys[mid] < first) lo = mid + 1;
                else hi = mid;
            }
            u64 bc = 0, bu = 0;
            long long bp = 0;
            for (long long j = lo; j < a.n_pairs && (a.keys[j] >> 32) == ti; ++j) {
                const long long pi = a.keys[j] & 0xffffffffll;
                if (pi < 1 || pi > a.n_p) continue;
                if (a.cls >= 0 && a.p_type != nullptr && a.p_type[pi - 1] != a.cls) continue;
                const u64 c = (u64)a.counts[j], bt = (u64)a.p_area[pi - 1], u = at + bt - c;
                v[S_D2_I] += (long long)c, v[S_D2_T] += (long long)(at + bt), v[S_D1_I] += (long long)c;
                if (2 * c > u) v[S_TP] += 1, iou = (double)c / (double)u;
                if (bp == 0 || im_mul_gt(c, bu, bc, u)) bp = pi, bc = c, bu = u;  // pairs come in ascending pred index: a tie keeps the smaller
            }
            if (bp != 0) v[S_AJI_I] += (long long)bc, v[S_AJI_U] += (long long)bu, a.used[bp - 1] = 1;
            else v[S_AJI_U] += (long long)at;
        }
        a.iou[ti - 1] = iou;
    }
    im_flush(a.summary, v, S_WORDS, threadIdx.x & 63);
}

__global__ __launch_bounds__(IM_BLOCK) void im_stats_pred_kernel(ImStats a) {
    long long v[S_WORDS];
    for (int i = 0; i < S_WORDS; ++i) v[i] = 0;
    for (long long i0 = blockIdx.x * (long long)IM_BLOCK; i0 < a.n_p; i0 += (long long)gridDim.x * IM_BLOCK) {
        const long long pi = i0 + threadIdx.x;
        if (pi >= a.n_p) continue;
        if (a.cls >= 0 && a.p_type != nullptr && a.p_type[pi] != a.cls) continue;
        v[S_NP] += 1, v[S_D1_T] += a.p_area[pi];
        if (!a.used[pi]) v[S_AJI_U] += a.p_area[pi];
    }
    im_flush(a.summary, v, S_WORDS, threadIdx.x & 63);
}

// one workgroup: the float64 sum in a fixed order (thread t adds elements t, t + 256, ... in turn; then a fixed tree), fp and fn from the counts
__global__ __launch_bounds__(IM_BLOCK) void im_stats_final_kernel(ImStats a) {
    __shared__ double part[IM_BLOCK];
    double s = 0.0;
    for (long long i = threadIdx.x; i < a.n_t; i += IM_BLOCK) s += a.iou[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = IM_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.sum_iou[0] = part[0];
        a.summary[S_FP] = a.summary[S_NP] - a.summary[S_TP];
        a.summary[S_FN] = a.summary[S_NT] - a.summary[S_TP];
    }
}

inline unsigned im_grid(long long n, long long per_block, long long cap) { return (unsigned)std::min(std::max((n + per_block - 1) / per_block, 1ll), cap); }
inline bool im_vec_ok(const void* p, long long stride) { return (uintptr_t)p % 16 == 0 && stride % 4 == 0; }

}  // namespace

extern "C" int cerb_inst_areas(const int32_t* labels, long long row_stride, int h, int w, int n_ids, long long* area, void* hip_stream) {
    if (labels == nullptr || area == nullptr || h < 1 || w < 1 || n_ids < 1 || n_ids > IM_MAX_IDS) return fail("cerb_inst_areas: bad arguments");
    if (row_stride < w) return fail("cerb_inst_areas: row stride below the width");
    const long long tx = ((long long)w + IM_TILE - 1) / IM_TILE, ty = ((long long)h + IM_TILE - 1) / IM_TILE, nt = tx * ty;
    const unsigned g = im_grid(nt, 1, 1 << 20);
    if (im_vec_ok(labels, row_stride))
        hipLaunchKernelGGL(im_area_kernel<true>, dim3(g), dim3(IM_BLOCK), 0, (hipStream_t)hip_stream, labels, row_stride, h, w, n_ids, tx, nt, (u64*)area);
    else
        hipLaunchKernelGGL(im_area_kernel<false>, dim3(g), dim3(IM_BLOCK), 0, (hipStream_t)hip_stream, labels, row_stride, h, w, n_ids, tx, nt, (u64*)area);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" size_t cerb_inst_pairs_workspace_bytes(long long capacity) {
    if (capacity < 1 || (capacity & (capacity - 1)) != 0 || capacity > (1ll << 34)) return 0;
    return (size_t)capacity * 16 + IM_META * 8;
}

extern "C" int cerb_inst_pairs(const int32_t* true_map, long long true_row_stride, const int32_t* pred_map, long long pred_row_stride, int h, int w,
                               const int32_t* true_index, int n_true_ids, const int32_t* pred_index, int n_pred_ids, void* table, long long capacity,
                               void* hip_stream) {
    if (true_map == nullptr || pred_map == nullptr || true_index == nullptr || pred_index == nullptr || table == nullptr) return fail("cerb_inst_pairs: null pointer");
    if (h < 1 || w < 1 || n_true_ids < 1 || n_pred_ids < 1 || n_true_ids > IM_MAX_IDS || n_pred_ids > IM_MAX_IDS) return fail("cerb_inst_pairs: empty map or id range");
    if (true_row_stride < w || pred_row_stride < w) return fail("cerb_inst_pairs: row stride below the width");
    const size_t bytes = cerb_inst_pairs_workspace_bytes(capacity);
    if (bytes == 0 || (uintptr_t)table % 8 != 0) return fail("cerb_inst_pairs: the capacity must be a power of two and the table 8-byte aligned");
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_OK(hipMemsetAsync(table, 0, bytes, st));
    ImTable tab;
    tab.meta = (u64*)table;
    tab.keys = tab.meta + IM_META;
    tab.counts = tab.keys + capacity;
    tab.mask = (u64)capacity - 1;
    const long long tx = ((long long)w + IM_TILE - 1) / IM_TILE, ty = ((long long)h + IM_TILE - 1) / IM_TILE, nt = tx * ty;
    // a persistent grid (eight blocks per CU's worth on a 256-CU part) walking the tiles: the per-block counters then cost a few thousand atomics in all
    const unsigned g = im_grid(nt, 1, 2048);
    if (im_vec_ok(true_map, true_row_stride) && im_vec_ok(pred_map, pred_row_stride))
        hipLaunchKernelGGL(im_pair_kernel<true>, dim3(g), dim3(IM_BLOCK), 0, st, true_map, true_row_stride, pred_map, pred_row_stride, h, w, true_index,
                           n_true_ids, pred_index, n_pred_ids, tx, nt, tab);
    else
        hipLaunchKernelGGL(im_pair_kernel<false>, dim3(g), dim3(IM_BLOCK), 0, st, true_map, true_row_stride, pred_map, pred_row_stride, h, w, true_index,
                           n_true_ids, pred_index, n_pred_ids, tx, nt, tab);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int cerb_inst_pairs_compact(const void* table, long long capacity, long long* keys_out, long long* counts_out, long long max_out,
                                       long long* n_out, void* hip_stream) {
    if (table == nullptr || keys_out == nullptr || counts_out == nullptr || n_out == nullptr || max_out < 1) return fail("cerb_inst_pairs_compact: bad arguments");
    if (cerb_inst_pairs_workspace_bytes(capacity) == 0) return fail("cerb_inst_pairs_compact: the capacity must be a power of two");
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_OK(hipMemsetAsync(n_out, 0, 8, st));
    const u64* keys = (const u64*)table + IM_META;
    hipLaunchKernelGGL(im_compact_kernel, dim3(im_grid(capacity, 256 * 8, 4096)), dim3(256), 0, st, keys, keys + capacity, capacity, keys_out, counts_out,
                       max_out, (u64*)n_out);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" size_t cerb_inst_pair_stats_workspace_bytes(int n_true, int n_pred) {
    return (size_t)std::max(n_true, 0) * 8 + (size_t)std::max(n_pred, 0) + 16;
}

extern "C" int cerb_inst_pair_stats(const long long* keys, const long long* counts, long long n_pairs, const long long* true_area, int n_true,
                                    const long long* pred_area, int n_pred, const int32_t* true_type, const int32_t* pred_type, int cls,
                                    long long* summary, double* sum_iou, void* ws, size_t ws_bytes, void* hip_stream) {
    if (summary == nullptr || sum_iou == nullptr || n_pairs < 0 || n_true < 0 || n_pred < 0) return fail("cerb_inst_pair_stats: bad arguments");
    if (n_pairs > 0 && (keys == nullptr || counts == nullptr)) return fail("cerb_inst_pair_stats: pairs without arrays");
    if ((n_true > 0 && true_area == nullptr) || (n_pred > 0 && pred_area == nullptr)) return fail("cerb_inst_pair_stats: instances without areas");
    if (cls >= 0 && ((n_true > 0 && true_type == nullptr) || (n_pred > 0 && pred_type == nullptr))) return fail("cerb_inst_pair_stats: a class filter needs both type vectors");
    if (ws == nullptr || ws_bytes < cerb_inst_pair_stats_workspace_bytes(n_true, n_pred) || (uintptr_t)ws % 8 != 0) return fail("cerb_inst_pair_stats: workspace too small or unaligned");
    hipStream_t st = (hipStream_t)hip_stream;
    ImStats a;
    a.keys = keys, a.counts = counts, a.n_pairs = n_pairs, a.t_area = true_area, a.p_area = pred_area;
    a.t_type = cls >= 0 ? true_type : nullptr, a.p_type = cls >= 0 ? pred_type : nullptr;
    a.n_t = n_true, a.n_p = n_pred, a.cls = cls < 0 ? -1 : cls;
    a.summary = summary, a.sum_iou = sum_iou;
    a.iou = (double*)ws;
    a.used = (unsigned char*)ws + (size_t)n_true * 8;
    HIP_OK(hipMemsetAsync(summary, 0, CERB_INST_SUMMARY_WORDS * 8, st));
    if (n_pred > 0) HIP_OK(hipMemsetAsync(a.used, 0, (size_t)n_pred, st));
    if (n_true > 0) hipLaunchKernelGGL(im_stats_true_kernel, dim3(im_grid(n_true, IM_BLOCK, 2048)), dim3(IM_BLOCK), 0, st, a);
    if (n_pred > 0) hipLaunchKernelGGL(im_stats_pred_kernel, dim3(im_grid(n_pred, IM_BLOCK, 2048)), dim3(IM_BLOCK), 0, st, a);
    hipLaunchKernelGGL(im_stats_final_kernel, dim3(1), dim3(IM_BLOCK), 0, st, a);
    HIP_OK(hipGetLastError());
    return 0;
}
