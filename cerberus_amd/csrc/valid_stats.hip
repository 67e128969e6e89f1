// Validation statistics on the device: the accumulator of the reference's ProcStepRawOutput callback (models/run_desc.py:606-747) over the read-outs
// of valid_step (:332-436), for all heads of a step in ONE grouped launch.
//
// blockIdx.y = head * N + sample: a sample whose flag byte is 0 (the head's name is not in its dummy_target row) leaves as a block.  A block walks
// its sample's H * W pixels in a grid-stride loop, four pixels per thread and step (16-byte loads: two float4 of an INST head's two probability
// channels, one 16-byte load of the true map; a TYPE head's uint8 class map is read 4 bytes at a time so that every load instruction of a wave
// covers one contiguous run), counts into uint32 registers -- per class k: inter, total, correct -- reduces them over the wave with cross-lane
// shuffles, over the block's waves through LDS, and adds each non-zero sum to the int64 accumulator [head][CERB_VALID_MAX_CLASSES][4] with one
// 64-bit atomicAdd per counter and block.  nr_pixels gets H * W once per flagged sample (block x = 0).
//
// Every count is an integer and integer addition is associative: the accumulator does not depend on the order in which blocks or lanes arrive and
// is bitwise reproducible from run to run.  No host synchronisation, no allocation; everything runs on the caller's stream.
//
// Arithmetic: class ids are compared as float32, the way numpy compares the reference's float32 'true' arrays with integer labels.  An int32 map is
// converted first -- exact for |id| < 2^24, which cerb_valid_stats_accumulate's contract asks for; ids beyond that never equal a class either way.
// NaN (a probability or a label) compares false with everything, as in numpy.
#include "cerb_net.h"

namespace {

constexpr int VS_MAXH = CERB_VALID_MAX_HEADS;
constexpr int VS_MAXC = CERB_VALID_MAX_CLASSES;
constexpr int VS_BLOCK = 256;
constexpr int VS_WAVES = VS_BLOCK / 64;
constexpr int VS_NCNT = 3 * VS_MAXC;  // per class: inter, total, correct

struct VsHeads {
    int n_heads;
    int kind[VS_MAXH];       // CERB_VALID_INST / _TYPE / _PATCH
    int classes[VS_MAXH];    // C: INST and TYPE count classes 1 .. C-1, Patch-Class 0 .. C-1
    int pred_fmt[VS_MAXH];   // TYPE: 0 uint8, 1 int64; Patch-Class: 0 map, 1 one float per sample
    int true_fmt[VS_MAXH];   // bit 0: float32 (else int32); bit 1: one value per sample
    int vec[VS_MAXH];        // 1: every pointer is 16-byte aligned and H * W % 4 == 0 -> the four-pixel path
    const void* pred[VS_MAXH];
    const void* tru[VS_MAXH];
};

struct VsCount {
    uint32_t inter[VS_MAXC], total[VS_MAXC], correct[VS_MAXC];
};

__device__ __forceinline__ float vs_true(uint32_t raw, bool is_float) { return is_float ? __uint_as_float(raw) : (float)(int32_t)raw; }
// an int64 class id as float: ids outside [0, 2^24) equal no class and no label
__device__ __forceinline__ float vs_id64(long long v) { return (v >= 0 && v < (1ll << 24)) ? (float)v : __uint_as_float(0x7fc00000u); }

// '*-INST' (run_desc.py:646-660): pred_ = (p[k-1] > 0.5) * k; inter = #(pred_ == k & true == k), total = #(pred_ == k) + #(true == k),
// correct = #(true == pred_) -- background agreeing with 0 included.
template <int NCH>
__device__ __forceinline__ void vs_inst(VsCount& c, const float* p, float t) {
#pragma unroll
    for (int k = 1; k <= NCH; ++k) {
        const bool pk = p[k - 1] > 0.5f, tk = (t == (float)k);
        c.inter[k] += (pk && tk) ? 1u : 0u;
        c.total[k] += (pk ? 1u : 0u) + (tk ? 1u : 0u);
        c.correct[k] += (pk ? tk : (t == 0.0f)) ? 1u : 0u;
    }
}
// '*-TYPE' (:661-674; MASKED = true: inter / total under true > 0, classes 1 ..) and Patch-Class (:675-686; unmasked, classes 0 ..);
// correct = #(true == pred), unmasked, one number for every class (kept in correct[0]).  The two class ids become one-hot bit masks once per
// pixel (0 for anything that is not one of the classes 0 .. 15: a label above the range, NaN) and every class takes its bit out of them: three
// bit-field extracts and adds per class and no compare, whose lane masks would otherwise fill the scalar registers.  KMAX: the classes below it
// are counted, so a head pays for the smallest of 3 / 9 / 16 that holds its classes.
__device__ __forceinline__ uint32_t vs_onehot(float v) {
    const int i = (int)fminf(fmaxf(v, -1.0f), (float)VS_MAXC);  // clamped first: the conversion is defined for every input (NaN -> -1)
    return (v == (float)i && i >= 0 && i < VS_MAXC) ? (1u << i) : 0u;
}
template <bool MASKED, int KMAX>
__device__ __forceinline__ void vs_class(VsCount& c, float p, float t) {
    const bool m = MASKED ? (t > 0.0f) : true;
    const uint32_t bp = m ? vs_onehot(p) : 0u, bt = m ? vs_onehot(t) : 0u, bi = bp & bt;
    c.correct[0] += (t == p) ? 1u : 0u;
#pragma unroll
    for (int k = MASKED ? 1 : 0; k < KMAX; ++k) {
        c.inter[k] += (bi >> k) & 1u;
        c.total[k] += ((bp >> k) & 1u) + ((bt >> k) & 1u);
    }
}

struct VsSample {  // one block's share: sample n of head hd
    const void* pred;
    const uint32_t* tr;  // the sample's true map (or its one value)
    int n, P, tid, nthr;
    bool vec, t_float, t_single;
    int pred_fmt;
};

template <int KMAX>
__device__ __forceinline__ void vs_type_pixels(VsCount& c, const VsSample& s) {
    const bool p64 = s.pred_fmt == 1;
    if (s.vec) {
        for (int g = s.tid; g < s.P / 4; g += s.nthr) {
            float p[4];
            if (p64) {
                const longlong2* q = (const longlong2*)((const long long*)s.pred + (long long)s.n * s.P) + 2 * g;
                const longlong2 a = q[0], b = q[1];
                p[0] = vs_id64(a.x), p[1] = vs_id64(a.y), p[2] = vs_id64(b.x), p[3] = vs_id64(b.y);
            } else {
                const uint32_t q = ((const uint32_t*)((const uint8_t*)s.pred + (long long)s.n * s.P))[g];
#pragma unroll
                for (int i = 0; i < 4; ++i) p[i] = (float)((q >> (8 * i)) & 255u);
            }
            const uint4 t4 = ((const uint4*)s.tr)[g];
            const uint32_t t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) vs_class<true, KMAX>(c, p[i], vs_true(t[i], s.t_float));
        }
    } else {
        for (int i = s.tid; i < s.P; i += s.nthr) {
            const float p = p64 ? vs_id64(((const long long*)s.pred)[(long long)s.n * s.P + i]) : (float)((const uint8_t*)s.pred)[(long long)s.n * s.P + i];
            vs_class<true, KMAX>(c, p, vs_true(s.tr[i], s.t_float));
        }
    }
}

// Patch-Class: the argmax spread over the tile (a map) or one value per sample, against a map or one value per sample
template <int KMAX>
__device__ __forceinline__ void vs_patch_pixels(VsCount& c, const VsSample& s) {
    const bool p_single = s.pred_fmt == 1;
    const float* pr = (const float*)s.pred + (p_single ? (long long)s.n : (long long)s.n * s.P);
    if (p_single && s.t_single) {  // H * W equal pixels: counted once, weighted by the caller
        if (s.tid == 0) vs_class<false, KMAX>(c, pr[0], vs_true(s.tr[0], s.t_float));
    } else if (s.vec && !p_single && !s.t_single) {
        for (int g = s.tid; g < s.P / 4; g += s.nthr) {
            const float4 a = ((const float4*)pr)[g];
            const uint4 t4 = ((const uint4*)s.tr)[g];
            const float p[4] = {a.x, a.y, a.z, a.w};
            const uint32_t t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) vs_class<false, KMAX>(c, p[i], vs_true(t[i], s.t_float));
        }
    } else {
        for (int i = s.tid; i < s.P; i += s.nthr) vs_class<false, KMAX>(c, pr[p_single ? 0 : i], vs_true(s.tr[s.t_single ? 0 : i], s.t_float));
    }
}

__device__ __forceinline__ uint32_t vs_wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(VS_BLOCK, 4) void vs_accumulate_kernel(VsHeads hs, const uint8_t* __restrict__ flags, int N, int P, unsigned long long* __restrict__ acc) {
    const int hd = blockIdx.y / N, n = blockIdx.y % N;
    if (flags[blockIdx.y] == 0) return;  // a dummy target: the whole block leaves
    const int kind = hs.kind[hd], C = hs.classes[hd];
    const bool t_float = hs.true_fmt[hd] & 1, t_single = hs.true_fmt[hd] & 2;
    const uint32_t* tr = (const uint32_t*)hs.tru[hd] + (t_single ? (long long)n : (long long)n * P);
    const int tid = blockIdx.x * VS_BLOCK + threadIdx.x, nthr = gridDim.x * VS_BLOCK;
    VsCount c;
#pragma unroll
    for (int k = 0; k < VS_MAXC; ++k) c.inter[k] = c.total[k] = c.correct[k] = 0;

    if (kind == CERB_VALID_INST && C == 3 && hs.vec[hd]) {  // what the network gives: two probability channels, interleaved
        const float4* pr = (const float4*)((const float*)hs.pred[hd] + (long long)n * P * 2);
        for (int g = tid; g < P / 4; g += nthr) {
            const float4 a = pr[2 * g], b = pr[2 * g + 1];
            const uint4 t4 = ((const uint4*)tr)[g];
            const float p[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            const uint32_t t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) vs_inst<2>(c, p + 2 * i, vs_true(t[i], t_float));
        }
    } else if (kind == CERB_VALID_INST) {  // any channel count, unaligned maps: one pixel per thread and step
        const int nch = C - 1;
        const float* pr = (const float*)hs.pred[hd] + (long long)n * P * nch;
        for (int i = tid; i < P; i += nthr) {
            float p[VS_MAXC - 1];
#pragma unroll
            for (int k = 0; k < VS_MAXC - 1; ++k) p[k] = k < nch ? pr[(long long)i * nch + k] : 0.0f;  // 0 is never > 0.5; classes >= C are not written
            vs_inst<VS_MAXC - 1>(c, p, vs_true(tr[i], t_float));
        }
    } else {
        const VsSample sm = {hs.pred[hd], tr, n, P, tid, nthr, hs.vec[hd] != 0, t_float, t_single, hs.pred_fmt[hd]};
        if (kind == CERB_VALID_TYPE) {
            if (C <= 3) vs_type_pixels<3>(c, sm);
            else if (C <= 9) vs_type_pixels<9>(c, sm);
            else vs_type_pixels<VS_MAXC>(c, sm);
        } else {
            if (C <= 3) vs_patch_pixels<3>(c, sm);
            else if (C <= 9) vs_patch_pixels<9>(c, sm);
            else vs_patch_pixels<VS_MAXC>(c, sm);
        }
    }

    // registers -> wave (shuffles) -> block (LDS) -> accumulator (one 64-bit atomic per non-zero counter)
    __shared__ uint32_t part[VS_WAVES][VS_NCNT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < VS_MAXC; ++k) {
        const uint32_t a = vs_wave_sum(c.inter[k]), b = vs_wave_sum(c.total[k]), d = vs_wave_sum(c.correct[k]);
        if (lane == 0) part[wave][3 * k] = a, part[wave][3 * k + 1] = b, part[wave][3 * k + 2] = d;
    }
    __syncthreads();
    if (threadIdx.x < VS_NCNT) {
        const int k = threadIdx.x / 3, s = threadIdx.x % 3;
        const int k0 = kind == CERB_VALID_PATCH ? 0 : 1;
        if (k >= k0 && k < C) {
            const int src = (s == 2 && kind != CERB_VALID_INST) ? 2 : threadIdx.x;  // TYPE / Patch-Class: correct is one number for every class
            unsigned long long v = 0;
#pragma unroll
            for (int w = 0; w < VS_WAVES; ++w) v += part[w][src];
            if (kind == CERB_VALID_PATCH && hs.pred_fmt[hd] == 1 && (hs.true_fmt[hd] & 2)) v *= (unsigned long long)P;
            unsigned long long* dst = acc + ((long long)hd * VS_MAXC + k) * 4;
            if (v) atomicAdd(dst + s, v);
            if (s == 0 && blockIdx.x == 0) atomicAdd(dst + 3, (unsigned long long)P);  // nr_pixels += H * W per flagged sample (:633,641)
        }
    }
}

}  // namespace

extern "C" size_t cerb_valid_stats_bytes(int n_heads) { return (size_t)std::max(n_heads, 0) * VS_MAXC * 4 * sizeof(int64_t); }

extern "C" int cerb_valid_stats_reset(int64_t* acc, int n_heads, void* hip_stream) {
    if (acc == nullptr || n_heads < 1) return fail("cerb_valid_stats_reset: no accumulator");
    HIP_OK(hipMemsetAsync(acc, 0, cerb_valid_stats_bytes(n_heads), (hipStream_t)hip_stream));
    return 0;
}

extern "C" int cerb_valid_stats_accumulate(const cerb_valid_heads* heads, const uint8_t* flags, int n, int h, int w, int64_t* acc, void* hip_stream) {
    if (heads == nullptr || heads->n_heads < 1 || heads->n_heads > VS_MAXH) return fail("cerb_valid_stats: 1.." + std::to_string(VS_MAXH) + " heads per call");
    if (flags == nullptr || acc == nullptr) return fail("cerb_valid_stats: flags and accumulator must be device pointers");
    if (n < 1 || h < 1 || w < 1) return fail("cerb_valid_stats: empty batch");
    const long long P = (long long)h * w;
    // per-block sums are uint32 (total counts up to 2 per pixel); sample offsets n * P * channels stay far inside int64
    if (P >= (1ll << 30) || (long long)n * heads->n_heads > 65535) return fail("cerb_valid_stats: batch too large for one call (h * w < 2^30, n * heads <= 65535)");
    VsHeads hs = {};
    hs.n_heads = heads->n_heads;
    for (int i = 0; i < hs.n_heads; ++i) {
        const int kind = heads->kind[i], C = heads->n_classes[i], pf = heads->pred_fmt[i], tf = heads->true_fmt[i];
        if (kind != CERB_VALID_INST && kind != CERB_VALID_TYPE && kind != CERB_VALID_PATCH) return fail("cerb_valid_stats: unknown head kind");
        if (C < (kind == CERB_VALID_PATCH ? 1 : 2) || C > VS_MAXC) return fail("cerb_valid_stats: 2.." + std::to_string(VS_MAXC) + " classes per head (Patch-Class: 1..)");
        if (heads->pred[i] == nullptr || heads->true_map[i] == nullptr) return fail("cerb_valid_stats: a head without prediction or true map");
        if (pf < 0 || pf > 1 || (kind == CERB_VALID_INST && pf != 0)) return fail("cerb_valid_stats: unknown prediction format");
        if (tf < 0 || tf > 3 || ((tf & 2) && kind != CERB_VALID_PATCH)) return fail("cerb_valid_stats: unknown true-map format (one value per sample is Patch-Class only)");
        hs.kind[i] = kind, hs.classes[i] = C, hs.pred_fmt[i] = pf, hs.true_fmt[i] = tf;
        hs.pred[i] = heads->pred[i], hs.tru[i] = heads->true_map[i];
        hs.vec[i] = (P % 4 == 0 && (uintptr_t)heads->pred[i] % 16 == 0 && (uintptr_t)heads->true_map[i] % 16 == 0) ? 1 : 0;
    }
    // about eight steps of four pixels per thread: the counters' reduction (144 shuffles per wave) is paid once per block
    const unsigned bx = (unsigned)std::min<long long>(std::max<long long>((P / 4 + VS_BLOCK * 8 - 1) / (VS_BLOCK * 8), 1), 64);
    hipLaunchKernelGGL(vs_accumulate_kernel, dim3(bx, (unsigned)(n * hs.n_heads)), dim3(VS_BLOCK), 0, (hipStream_t)hip_stream, hs, flags, n, (int)P,
                       (unsigned long long*)acc);
    HIP_OK(hipGetLastError());
    return 0;
}
