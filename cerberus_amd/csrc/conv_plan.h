// Which kernel a convolution of the schedules takes, and the profile family it is reported under: THE rule, in one place.  run_conv (cerb_api.hip)
// launches by it, the taped forward of cerb_net_train_grads (cerb_train.hip) asks it whether a layer's kernel has a BatchNorm statistics stage, and
// the data gradient calls it with the channel roles swapped.  Plain C++17, no HIP: tests/test_conv_plan_host.py compiles it by itself.
#ifndef CERB_CONV_PLAN_H
#define CERB_CONV_PLAN_H
#include <string>

enum ConvKernel {
    CONV_IGEMM,         // conv_igemm.hip: direct implicit GEMM (every 1x1 and stride-2 convolution; conv_algo 0)
    CONV_IGEMM_PLANAR,  // ... with the tile-planar epilogue: a planar encoder stage's stride-2 entry, NHWC in, tile-planar out
    CONV_WINO2,         // conv_wino.hip: Winograd F(2x2,3x3)
    CONV_WINO4,         // conv_wino4.hip: F(4x4,3x3), two-block items (half the weight traffic)
    CONV_WINO4B,        // conv_wino4b.hip: F(4x4,3x3), one-block items, 32-channel chunks
    CONV_WINO4P,        // conv_wino4p.hip: F(4x4,3x3) on tile-planar tensors
    CONV_NONE           // a tile-planar launch was asked for where no kernel can serve it: an internal error of the schedule
};

// Where a tile-planar launch sits: the decoder level 0..3, or an encoder stage (the only planar launches with a residual, and with stride-2 producers).
// Names the kernel symbol (ConvParams::level_tag) and the profile family.
enum { kSiteEncoder = 4 };

struct ConvLayer {
    int conv_algo;      // cerb_net_set_conv_algo: 0, 1, 5, 6, 7
    int ks, stride;
    int cin, cout;      // contraction and output channels (the data gradient swaps the layer's two)
    int ho, wo;         // output map
    bool wino;          // Winograd-packed: F(2x2) weights exist for this role (3x3, stride 1 as a convolution, channel counts the kernels take)
    int mode;           // conv_igemm.hip's input mode; != 0 (skip + upsampled prev summed on the load) only the direct kernel has
    bool planar;        // in / out tile-planar (a stride-2 convolution: out only)
    bool train_packed;  // raw weights, BatchNorm apart (cerb_net_set_fold_bn(net, 0)): the planar kernels' epilogues do not serve it
};

constexpr long long kF4MinPx = 256;    // 16 x 16: the smallest map F(4x4) takes under conv_algo 6
constexpr long long kW4bMaxPx = 4096;  // 64 x 64: the largest map conv_wino4b takes under conv_algo 6; conv_wino4 (and the planar decoder levels) from there

// conv_algo 6 (default): F(4x4,3x3) for maps of at least 16 x 16 pixels -- conv_wino4b.hip (one-block items, 32-channel chunks) up to
// 64 x 64, conv_wino4.hip (two-block items, half the weight traffic) above; F(2x2,3x3) for smaller maps, where a 16 x 16 block would
// be mostly padding.  Measured per layer on a batch of 32 256-pixel tiles (scripts/dev_conv_layers.py): 16^2 x 512 ch 0.115 / 0.21 /
// 0.146 ms (4b / 4 / F(2x2)), 64^2 x 128 ch 0.131 / 0.138 / 0.158, 256^2 x 64 ch x 5 decoders 2.63 / 2.52 / 3.28.  5 / 7: F(4x4) on every
// map with conv_wino4 / conv_wino4b (7: where the contraction is whole 64-channel blocks), 1: F(2x2), 0: direct.
// The rule looks at the layer's geometry only -- never at the batch size or the region of interest -- so that a tile's values do not depend
// on what it is batched with (sharded == unsharded, cropped == full stay bitwise, tests/test_drivers_gpu.py, test_net_gpu.py).
inline ConvKernel conv_plan(const ConvLayer& l) {
    const long long px = (long long)l.ho * l.wo;
    const bool wino = l.wino && l.ks == 3 && l.stride == 1 && l.cout % 64 == 0 && l.mode == 0;
    const bool f4 = wino && (l.conv_algo == 5 || l.conv_algo == 7 || (l.conv_algo == 6 && px >= kF4MinPx));
    if (l.planar) {
        if (l.train_packed || l.mode != 0) return CONV_NONE;
        if (l.stride == 2) return CONV_IGEMM_PLANAR;
        return f4 ? CONV_WINO4P : CONV_NONE;
    }
    if (f4) return (l.conv_algo == 7 || (l.conv_algo == 6 && px <= kW4bMaxPx)) && l.cin % 64 == 0 ? CONV_WINO4B : CONV_WINO4;
    return wino && l.conv_algo ? CONV_WINO2 : CONV_IGEMM;
}

// the F(4x4) kernels on NHWC maps leave BatchNorm statistics partials from their output stage (ConvParams::bn_part); the others have no such stage
inline bool conv_has_bn_stats(ConvKernel k) { return k == CONV_WINO4 || k == CONV_WINO4B; }

// Profile family of a launch (cerb_net_profile_get; bench.py prices executed FLOPs by these prefixes and keeps the decoder levels apart).
// packed_items: conv_wino4b takes 16 consecutive tiles per item on this map (cerb_wino4b_packed); site: of a tile-planar launch.
// The two lowest decoder levels' names start with "conv_wino4_planar", not "conv_wino4p": tests/test_net_gpu.py counts the families that start with
// "conv_wino4p" and expects the two last levels' four launches.  The encoder's planar stages start with "conv_wino4" and with none of the decoder's prefixes.
// The data gradient reports the same names behind "dgrad:".
inline std::string conv_family(ConvKernel k, const ConvLayer& l, bool has_resid, bool packed_items, int site) {
    static const char* const kPlanarFamily[4] = {"conv_wino4_planar<f4x4,16x16x2,eighth-res>", "conv_wino4_planar<f4x4,16x16x2,quarter-res>",
                                              "conv_wino4p<f4x4,16x16x2,planar,half-res>", "conv_wino4p<f4x4,16x16x2,planar>"};
    const std::string res = has_resid ? ",res>" : ">", blk = l.wo < 32 ? ",16x16>" : ",8x32>";
    switch (k) {
        case CONV_WINO4P: return site == kSiteEncoder ? "conv_wino4_enc<f4x4,16x16x2" + res : kPlanarFamily[site];  // (run_conv: a planar launch names its site)
        case CONV_WINO4B: return (packed_items ? "conv_wino4b<f4x4,16t" : "conv_wino4b<f4x4,16x16") + res;
        case CONV_WINO4: return "conv_wino4<f4x4,16x16x2" + res;
        case CONV_WINO2: return "conv_wino<f2x2,8x16" + res;
        case CONV_IGEMM_PLANAR: return "conv_igemm_planar<ks" + std::to_string(l.ks) + ",s2" + blk;
        default: return "conv_igemm<ks" + std::to_string(l.ks) + ",s" + std::to_string(l.stride) + ",mode" + std::to_string(l.mode) + blk;
    }
}
#endif  // CERB_CONV_PLAN_H
