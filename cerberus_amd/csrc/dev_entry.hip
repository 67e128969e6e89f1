// dev_entry.hip -- test-only entry layer, linked into libcerberus_hip_dev.so ONLY (cerberus_amd/build.py: DEV_ONLY_SOURCES).  The backward kernels of
// the training step are reachable in the product only through cerb_net_train_grads; these thin wrappers let tests/test_kernel_parity_gpu.py call one
// launcher of cerb_net.h at a time, on raw device pointers, and compare it with a float64 reference of the same operation (tests/kernel_refs.py);
// the cerb_devfwd_* entries do the same for the forward path (convolutions, stem, output heads, Patch-Class, decoder entry, pool, layout).
// No logic beyond argument checks: every wrapper returns the launcher's hipError_t as an int (0 = hipSuccess, 1 = hipErrorInvalidValue for a bad
// argument).  Not part of the boundary: include/cerberus_hip.h declares none of this and libcerberus_hip.so exports none of it (tests/test_abi.py).
#include "cerb_net.h"

#define DEV_NEED(cond) \
    do {               \
        if (!(cond)) return (int)hipErrorInvalidValue; \
    } while (0)

extern "C" {

// ---- Winograd-domain weight gradient (conv_wgrad_wino.hip) ----------------------------------------------------------------------------------------
int cerb_dev_wgrad_wino_supported(int H, int W, int Cin, int Cout) { return cerb_wgrad_wino_supported(H, W, Cin, Cout) ? 1 : 0; }
size_t cerb_dev_wgrad_wino_workspace_bytes(int G, int N, int H, int W, int Cin, int Cout) {
    return cerb_wgrad_wino_supported(H, W, Cin, Cout) ? cerb_wgrad_wino_workspace_bytes(G, N, H, W, Cin, Cout) : 0;
}
int cerb_dev_wgrad_wino(const float* x, const float* dy, float* dw, float* db, int G, int N, int H, int W, int Cin, int Cout, long long x_gs, void* ws, void* st) {
    DEV_NEED(x && dy && dw && ws && G > 0 && N > 0);
    return (int)cerb_launch_wgrad_wino(x, dy, dw, G, N, H, W, Cin, Cout, x_gs, ws, (hipStream_t)st, db);
}

// ---- direct weight gradient (conv_wgrad.hip); Ho / Wo are the OUTPUT map of the convolution ------------------------------------------------------
size_t cerb_dev_wgrad_workspace_bytes(int G, int N, int Ho, int Wo, int Cin, int Cout, int ks, int* slices_out) {
    return cerb_wgrad_workspace_bytes(G, N, Ho, Wo, Cin, Cout, ks, slices_out);
}
int cerb_dev_wgrad(const float* x, const float* dy, float* dw, float* db, int G, int N, int H, int W, int Cin, int Cout, int ks, int stride, long long x_gs, void* ws,
                   void* st) {
    DEV_NEED(x && dy && dw && ws && G > 0 && N > 0 && H > 0 && W > 0);
    return (int)cerb_launch_wgrad(x, dy, dw, G, N, H, W, Cin, Cout, ks, stride, x_gs, ws, (hipStream_t)st, db);
}

// ---- the 7x7 stem on uint8 tiles ---------------------------------------------------------------------------------------------------------------
size_t cerb_dev_stem_wgrad_mfma_workspace_bytes() { return cerb_stem_wgrad_workspace_bytes(); }
int cerb_dev_stem_wgrad_mfma(const unsigned char* tiles, const float* dy, float* dw, int N, int H, int W, void* ws, void* st) {
    DEV_NEED(tiles && dy && dw && ws && N > 0 && H > 0 && W > 0);
    return (int)cerb_launch_stem_wgrad_mfma(tiles, dy, dw, N, H, W, ws, (hipStream_t)st);
}
int cerb_dev_stem_wgrad(const unsigned char* tiles, const float* dy, float* dw, int N, int H, int W, void* st) {
    DEV_NEED(tiles && dy && dw && N > 0 && H > 0 && W > 0);
    return (int)cerb_launch_stem_wgrad(tiles, dy, dw, N, H, W, (hipStream_t)st);
}

// ---- gather-form convolution backward (the fallback behind conv_algo 0): dx accumulated, dw / db assigned; any of the three may be null ---------
int cerb_dev_conv_bwd(const float* x, const float* dy, const float* w, float* dx, float* dw, float* db, int G, int N, int H, int W, int Cin, int Cout, int ks, int stride,
                      long long x_gs, void* st) {
    DEV_NEED(dy && (dx || dw || db) && (!dx || w) && (!dw || x) && G > 0 && N > 0 && (ks == 1 || ks == 3) && (stride == 1 || stride == 2));
    return (int)cerb_launch_conv_bwd(x, dy, w, dx, dw, db, G, N, H, W, Cin, Cout, ks, stride, x_gs, (hipStream_t)st);
}

// ---- BatchNorm: statistics, finalise from partials, backward -----------------------------------------------------------------------------------
size_t cerb_dev_bn_workspace_bytes(int groups, long long rows, int C) { return cerb_bn_workspace_bytes(groups, rows, C); }
size_t cerb_dev_bn_fold_workspace_bytes(int groups, int C) { return cerb_bn_fold_workspace_bytes(groups, C); }
int cerb_dev_bn_stats(const float* x, long long group_stride, long long rows, int C, int groups, float eps, float* mean, float* rstd, float* var_unbiased, void* ws,
                      void* st) {
    DEV_NEED(x && mean && rstd && ws && rows > 0 && groups > 0);
    return (int)cerb_launch_bn_stats(x, group_stride, rows, C, groups, eps, mean, rstd, var_unbiased, ws, (hipStream_t)st);
}
int cerb_dev_bn_finalize(const double* partial, int blocks, long long rows, int C, float eps, float* mean, float* rstd, float* var_unbiased, int groups, void* fold_ws,
                         void* st) {
    DEV_NEED(partial && mean && rstd && blocks > 0 && rows > 0 && groups > 0);
    return (int)cerb_launch_bn_finalize(partial, blocks, rows, C, eps, mean, rstd, var_unbiased, (hipStream_t)st, groups, fold_ws);
}
int cerb_dev_bn_bwd(const float* dz, const float* z, const float* y, float* dy, float* dresid, long long group_stride, long long rows, int C, int groups, const float* mean,
                    const float* rstd, const float* gamma, const float* beta, float* dgamma, float* dbeta, int relu, int dy_assign, int dresid_assign,
                    unsigned long long eval_mask, void* ws, void* st) {
    DEV_NEED(dz && y && dy && mean && rstd && gamma && dgamma && dbeta && ws && rows > 0 && groups > 0 && (!relu || z || (beta && !dresid)));
    return (int)cerb_launch_bn_bwd(dz, z, y, dy, dresid, group_stride, rows, C, groups, mean, rstd, gamma, beta, dgamma, dbeta, relu, dy_assign, ws, (hipStream_t)st, eval_mask,
                                   dresid_assign);
}

// ---- decoder entry: out_g = skip + up2(prev_g) ---------------------------------------------------------------------------------------------------
int cerb_dev_upadd_bwd_fused_ok(int H, int W, int C, int G) { return cerb_upadd_bwd_fused_ok(H, W, C, G) ? 1 : 0; }
int cerb_dev_upadd_bwd(const float* dout, float* dskip, float* dprev, int G, int N, int H, int W, int C, long long prev_gs, int shared_prev, unsigned group_mask,
                       int skip_assign, int prev_assign, void* st) {
    DEV_NEED(dout && dskip && dprev && G > 0 && N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C % 4 == 0);
    return (int)cerb_launch_upadd_bwd(dout, dskip, dprev, G, N, H, W, C, prev_gs, shared_prev, (hipStream_t)st, group_mask, skip_assign, prev_assign);
}

// ---- max-pool 3x3 / 2 / 1 ------------------------------------------------------------------------------------------------------------------------
int cerb_dev_maxpool_idx(const float* in, float* out, unsigned* idx, int N, int H, int W, int C, void* st) {
    DEV_NEED(in && out && idx && N > 0 && H > 0 && W > 0 && C % 4 == 0);
    return (int)cerb_launch_maxpool_idx(in, out, idx, N, H, W, C, (hipStream_t)st);
}
int cerb_dev_maxpool_bwd_idx(const unsigned* idx, const float* dy, float* dx, int N, int H, int W, int C, void* st) {
    DEV_NEED(idx && dy && dx && N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C % 4 == 0);
    return (int)cerb_launch_maxpool_bwd_idx(idx, dy, dx, N, H, W, C, (hipStream_t)st);
}
int cerb_dev_maxpool_bwd(const float* x, const float* ypool, const float* dy, float* dx, int N, int H, int W, int C, void* st) {
    DEV_NEED(x && ypool && dy && dx && N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C % 4 == 0);
    return (int)cerb_launch_maxpool_bwd(x, ypool, dy, dx, N, H, W, C, (hipStream_t)st);
}

// ---- pointwise layers -----------------------------------------------------------------------------------------------------------------------------
int cerb_dev_pointwise_bwd(const float* x, const float* dy, const float* w, float* dx, float* dw, float* db, long long rows, int cin, int cout, const float* in_scale,
                           int dx_assign, void* st) {
    DEV_NEED(dy && (dx || dw || db) && (!dx || w) && (!dw || x) && rows > 0 && cin > 0 && cout > 0);
    return (int)cerb_launch_pointwise_bwd(x, dy, w, dx, dw, db, rows, cin, cout, in_scale, dx_assign, (hipStream_t)st);
}
size_t cerb_dev_pw_bwd_small_workspace_bytes(long long rows, int cin, int cout) { return cerb_pw_bwd_small_workspace_bytes(rows, cin, cout); }
int cerb_dev_pw_bwd_small(const float* x, const float* dy, const float* w, float* dx, float* dw, float* db, long long rows, int cin, int cout, int dx_assign, void* ws,
                          void* st) {
    DEV_NEED(x && dy && w && ws && rows > 0 && cin > 0 && cout > 0);
    return (int)cerb_launch_pw_bwd_small(x, dy, w, dx, dw, db, rows, cin, cout, dx_assign, ws, (hipStream_t)st);
}
size_t cerb_dev_pw_wgrad_small_workspace_bytes(long long rows, int cin, int cout) { return cerb_pw_wgrad_small_workspace_bytes(rows, cin, cout); }
int cerb_dev_pw_wgrad_small(const float* x, const float* dy, float* dw, long long rows, int cin, int cout, void* ws, void* st) {
    DEV_NEED(x && dy && dw && ws && rows > 0 && cin > 0 && cout > 0);
    return (int)cerb_launch_pw_wgrad_small(x, dy, dw, rows, cin, cout, ws, (hipStream_t)st);
}

// ---- column sums, centre crop + average pool, stride-2 dilation --------------------------------------------------------------------------------
// (the schedule hands cerb_launch_colsum its large shared workspace; the launcher uses [G][slabs <= 2048][C] floats of it)
size_t cerb_dev_colsum_workspace_bytes(int C, int G) { return (size_t)G * 2048 * C * 4; }
int cerb_dev_colsum(const float* d, long long group_stride, long long rows, int C, int G, float* out, void* ws, void* st) {
    DEV_NEED(d && out && ws && rows > 0 && C > 0 && G > 0);
    return (int)cerb_launch_colsum(d, group_stride, rows, C, G, out, ws, (hipStream_t)st);
}
int cerb_dev_crop_gap(const float* x, int N, int H, int W, int C, int y0, int ch, int x0, int cw, float* out, void* st) {
    DEV_NEED(x && out && N > 0 && C > 0 && y0 >= 0 && x0 >= 0 && ch > 0 && cw > 0 && y0 + ch <= H && x0 + cw <= W);
    return (int)cerb_launch_crop_gap(x, N, H, W, C, y0, ch, x0, cw, out, (hipStream_t)st);
}
int cerb_dev_crop_gap_bwd(const float* dg, float* dx, int N, int H, int W, int C, int y0, int ch, int x0, int cw, void* st) {
    DEV_NEED(dg && dx && N > 0 && C > 0 && y0 >= 0 && x0 >= 0 && ch > 0 && cw > 0 && y0 + ch <= H && x0 + cw <= W);
    return (int)cerb_launch_crop_gap_bwd(dg, dx, N, H, W, C, y0, ch, x0, cw, (hipStream_t)st);
}
int cerb_dev_dilate2(const float* dy, float* d, long long n, int H, int W, int C, void* st) {
    DEV_NEED(dy && d && n > 0 && H > 0 && W > 0);
    return (int)cerb_launch_dilate2(dy, d, n, H, W, C, (hipStream_t)st);
}

// ---- forward decoder entry, NHWC and tile-planar (bound by tests/test_decoder_low_planar_gpu.py itself: the forward path's launchers are otherwise reached
// through cerb_net_forward only).  `out` of the planar form is a tile-planar tensor (cerb_common.h) of cerb_devfwd_planar_elems floats per group --------
long long cerb_devfwd_planar_elems(int N, int H, int W, int C) { return cerb_planar_elems(N, H, W, C); }
int cerb_devfwd_upsample2_add(const float* skip, const float* prev, float* out, int G, int N, int H, int W, int C, long long prev_gs, void* st) {
    DEV_NEED(skip && prev && out && G > 0 && N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C % 4 == 0);
    return (int)cerb_launch_upsample2_add(skip, prev, out, G, N, H, W, C, prev_gs, nullptr, (hipStream_t)st);
}
int cerb_devfwd_upsample2_add_planar(const float* skip, const float* prev, float* out, int G, int N, int H, int W, int C, long long prev_gs, long long out_gs,
                                     int prev_planar, void* st) {
    DEV_NEED(skip && prev && out && G > 0 && N > 0 && H > 0 && W > 0 && out_gs >= cerb_planar_elems(N, H, W, C));
    return (int)cerb_launch_upsample2_add_planar(skip, prev, out, G, N, H, W, C, prev_gs, out_gs, nullptr, prev_planar, (hipStream_t)st);
}

// ---- the encoder's tile-planar stages (bound by tests/test_encoder_planar_gpu.py): one launch at a time, NHWC against tile-planar.  The convolutions take
// HOST weights [Cout][Cin][k][k] (BatchNorm already folded), pack them as the handle would, and free the packed copy before they return ---------------
static int devfwd_upload(const std::vector<float>& v, float** out) {
    if (hipMalloc((void**)out, v.size() * 4) != hipSuccess) return 1;
    return hipMemcpy(*out, v.data(), v.size() * 4, hipMemcpyHostToDevice) != hipSuccess;
}
// 3x3 stride 1 (+ bias, + residual, ReLU): planar = 0 conv_wino4b.hip on NHWC tensors, 1 conv_wino4p.hip on tile-planar ones (`out` may be `resid`)
int cerb_devfwd_conv3x3(const float* w_host, const float* bias, const float* in, const float* resid, float* out, int N, int H, int W, int Cin, int Cout, int relu,
                        int planar, void* st) {
    DEV_NEED(w_host && bias && in && out && N > 0 && H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0 && Cin % 64 == 0 && Cout % 64 == 0);
    std::vector<float> w4;
    cerb_host_pack_wino4(w_host, Cout, Cin, planar ? 0 : 1, &w4);
    float* dw = nullptr;
    DEV_NEED(devfwd_upload(w4, &dw) == 0);
    ConvParams p;
    memset(&p, 0, sizeof(p));
    p.in = in; p.wpack = dw; p.bias = bias; p.resid = resid; p.out = out;
    p.N = N; p.H = p.Ho = H; p.W = p.Wo = W; p.Cin = Cin; p.Cout = Cout; p.relu = relu; p.groups = 1;
    p.w_gs = (long long)Cout * Cin * 36; p.bias_gs = Cout; p.pk_off = 1;
    p.out_gs = planar ? cerb_planar_elems(N, H, W, Cout) : (long long)N * H * W * Cout;
    if (planar) {
        p.level_tag = resid ? 4 : 3;
        p.pl_byp = cerb_planar_blocks(H);
        p.pl_bxp = cerb_planar_blocks(W);
    }
    hipError_t e = planar ? cerb_launch_wino4p(p, (hipStream_t)st) : cerb_launch_wino4b(p, (hipStream_t)st);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)st);
    (void)hipFree(dw);
    return (int)e;
}
// 3x3 or 1x1 stride 2 (+ bias, ReLU as asked) from an NHWC input: planar = 0 NHWC output, 1 tile-planar output (conv_igemm.hip's planar epilogue)
int cerb_devfwd_conv_s2(const float* w_host, const float* bias, const float* in, float* out, int N, int H, int W, int Cin, int Cout, int ks, int relu, int planar, void* st) {
    DEV_NEED(w_host && bias && in && out && N > 0 && H % 32 == 0 && W % 32 == 0 && Cin % 16 == 0 && Cout % 64 == 0 && (ks == 1 || ks == 3));
    std::vector<float> wp;
    cerb_host_pack_conv(w_host, Cout, Cin, ks, cerb_conv_chunk(ks, 2), &wp);
    float* dw = nullptr;
    DEV_NEED(devfwd_upload(wp, &dw) == 0);
    ConvParams p;
    memset(&p, 0, sizeof(p));
    p.in = in; p.wpack = dw; p.bias = bias; p.out = out;
    p.N = N; p.H = H; p.W = W; p.Ho = H / 2; p.Wo = W / 2; p.Cin = Cin; p.Cout = Cout; p.relu = relu; p.groups = 1;
    p.w_gs = (long long)Cout * Cin * ks * ks; p.bias_gs = Cout;
    p.out_gs = planar ? cerb_planar_elems(N, p.Ho, p.Wo, Cout) : (long long)N * p.Ho * p.Wo * Cout;
    if (planar) {
        p.pl_byp = cerb_planar_blocks(p.Ho);
        p.pl_bxp = cerb_planar_blocks(p.Wo);
    }
    hipError_t e = cerb_launch_conv(p, ks, 2, 0, (hipStream_t)st);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)st);
    (void)hipFree(dw);
    return (int)e;
}
// ---- every forward convolution launcher on its own (tests/test_conv_forward_parity_gpu.py), the data-gradient use of cerb_train.hip included.
// launcher: 0 cerb_launch_conv (ks 1 / 3, stride 1 / 2, mode 0 / 1), 1 cerb_launch_wino, 2 cerb_launch_wino4, 3 cerb_launch_wino4b, 4 cerb_launch_wino4p
// (level_tag 0..4, pl_byp / pl_bxp as given; a non-zero pl_byp with launcher 0 asks for conv_igemm's planar epilogue).  w_raw: DEVICE weights
// [G][Cout][Cin][k][k] (dgrad = 1: the forward layer's tensor, [G][Cin][Cout][3][3] in this launch's channel counts), packed here by the device packer the
// schedule uses for that launcher (host_pack = 0; dgrad as given) or by the host packer (host_pack = 1, dgrad = 0 only); w_gs follows from the packer.
// roi: four HOST ints (y0, y1, x0, x1) or null.  Checks what the launchers document and do not check themselves, and every channel constraint before a packer runs (the packers index whole chunks and blocks of w_raw); a launcher's error is the return code.
// Synchronises and frees the packed copy before it returns.
int cerb_devfwd_conv(int launcher, int ks, int stride, int mode, int level_tag, const float* w_raw, int host_pack, int dgrad, const float* in, const float* prev,
                     const float* bias, const float* resid, float* out, double* bn_part, int G, int N, int H, int W, int Cin, int Cout, int relu, long long in_gs,
                     long long prev_gs, long long bias_gs, long long resid_gs, long long out_gs, const int* roi, int pk_off, int pl_byp, int pl_bxp, void* st) {
    DEV_NEED(launcher >= 0 && launcher <= 4 && w_raw && in && bias && out && G > 0 && N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0);
    DEV_NEED(!(host_pack && dgrad) && (!bn_part || launcher == 2 || launcher == 3) && ((mode == 1) == (prev != nullptr)));
    if (launcher == 0) {  // conv_igemm.hip: whole chunks and whole 64-channel output blocks, no region of interest, no data-gradient packer
        DEV_NEED((ks == 1 || ks == 3) && (stride == 1 || stride == 2) && (mode == 0 || (mode == 1 && ks == 3 && stride == 1 && H % 2 == 0 && W % 2 == 0)));
        DEV_NEED(Cin % cerb_conv_chunk(ks, stride) == 0 && Cout % 64 == 0 && !roi && !dgrad && (stride == 1 || (H % 2 == 0 && W % 2 == 0)));
    } else {  // the Winograd launchers' own channel constraints, BEFORE anything is packed: the packers index whole chunks and whole 64-channel blocks of w_raw
        DEV_NEED(ks == 3 && stride == 1 && mode == 0 && Cin % ((launcher == 1 || launcher == 3) ? 32 : 16) == 0 && Cout % 64 == 0);
    }
    const hipStream_t s = (hipStream_t)st;
    const int taps = launcher == 0 ? ks * ks : (launcher == 1 ? 16 : 36);
    const size_t nw = (size_t)Cout * Cin * ks * ks, nu = (size_t)Cout * Cin * taps;
    float* dw = nullptr;
    hipError_t e = hipSuccess;
    if (host_pack) {
        std::vector<float> raw(nw * G), pk;
        DEV_NEED(hipMemcpy(raw.data(), w_raw, raw.size() * 4, hipMemcpyDeviceToHost) == hipSuccess);
        for (int g = 0; g < G; ++g) {
            if (launcher == 0) cerb_host_pack_conv(raw.data() + g * nw, Cout, Cin, ks, cerb_conv_chunk(ks, stride), &pk);
            else if (launcher == 1) cerb_host_pack_wino(raw.data() + g * nw, Cout, Cin, &pk);
            else cerb_host_pack_wino4(raw.data() + g * nw, Cout, Cin, launcher == 3 ? 1 : 0, &pk);
        }
        DEV_NEED(pk.size() == nu * G && devfwd_upload(pk, &dw) == 0);
    } else {
        DEV_NEED(hipMalloc((void**)&dw, nu * G * 4) == hipSuccess);
        if (launcher >= 2) {
            e = cerb_launch_pack_wino4(w_raw, dw, Cout, Cin, dgrad, launcher == 3 ? 1 : 0, G, s);
        } else {
            for (int g = 0; g < G && e == hipSuccess; ++g)
                e = launcher == 0 ? cerb_launch_pack_conv(w_raw + g * nw, dw + g * nu, Cout, Cin, ks, cerb_conv_chunk(ks, stride), s)
                                  : cerb_launch_pack_wino(w_raw + g * nw, dw + g * nu, Cout, Cin, dgrad, s);
        }
    }
    ConvParams p;
    memset(&p, 0, sizeof(p));
    p.in = in; p.prev = prev; p.wpack = dw; p.bias = bias; p.resid = resid; p.out = out; p.bn_part = bn_part;
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.relu = relu; p.groups = G;
    p.Ho = stride == 2 ? H / 2 : H;
    p.Wo = stride == 2 ? W / 2 : W;
    p.in_gs = in_gs; p.prev_gs = prev_gs; p.w_gs = (long long)nu; p.bias_gs = bias_gs; p.resid_gs = resid_gs; p.out_gs = out_gs;
    if (roi) { p.roi_y0 = roi[0]; p.roi_y1 = roi[1]; p.roi_x0 = roi[2]; p.roi_x1 = roi[3]; }
    p.pk_off = pk_off; p.level_tag = level_tag; p.pl_byp = pl_byp; p.pl_bxp = pl_bxp;
    if (e == hipSuccess) {
        switch (launcher) {
            case 0: e = cerb_launch_conv(p, ks, stride, mode, s); break;
            case 1: e = cerb_launch_wino(p, s); break;
            case 2: e = cerb_launch_wino4(p, s); break;
            case 3: e = cerb_launch_wino4b(p, s); break;
            default: e = cerb_launch_wino4p(p, s); break;
        }
    }
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
    (void)hipFree(dw);
    return (int)e;
}
static ConvParams devfwd_geom(int N, int H, int W, int Cin, int Cout, int pk_off) {
    ConvParams q;
    memset(&q, 0, sizeof(q));
    q.N = N; q.H = q.Ho = H; q.W = q.Wo = W; q.Cin = Cin; q.Cout = Cout; q.pk_off = pk_off;
    return q;
}
// conv_wino4b's item form for a whole-map launch of this geometry, and the BatchNorm partial rows per group it leaves
int cerb_devfwd_wino4b_packed(int N, int H, int W, int Cin, int Cout, int pk_off) { return cerb_wino4b_packed(devfwd_geom(N, H, W, Cin, Cout, pk_off)) ? 1 : 0; }
int cerb_devfwd_wino4b_bn_blocks(int N, int H, int W, int Cin, int Cout, int pk_off) { return cerb_wino4b_bn_blocks(devfwd_geom(N, H, W, Cin, Cout, pk_off)); }

int cerb_devfwd_maxpool(const float* in, float* out, int N, int H, int W, int C, int planar, void* st) {
    DEV_NEED(in && out && N > 0 && H > 0 && W > 0 && C % 4 == 0);
    return (int)(planar ? cerb_launch_maxpool_planar(in, out, N, H, W, C, (hipStream_t)st) : cerb_launch_maxpool(in, out, N, H, W, C, (hipStream_t)st));
}
int cerb_devfwd_planar_to_nhwc(const float* in, float* out, int N, int H, int W, int C, void* st) {
    DEV_NEED(in && out && N > 0);
    return (int)cerb_launch_planar_to_nhwc(in, out, N, H, W, C, (hipStream_t)st);
}

// ---- what lies between the convolutions and the user (tests/test_net_kernels_parity_gpu.py): stem, output heads, Patch-Class, the decoder entry with
// a region of interest.  Weights arrive RAW, as the state dict holds them, and are packed here by the functions cerb_net_finalize packs with ---------
// stem: tiles uint8 [N][H][W][3] or tiles_f32 (exactly one); w_raw DEVICE [64][3][7][7]; scale / shift HOST [64].  host_pack = 0: cerb_launch_pack_stem
// (a training handle's packer: no scale, so scale must be 1), 1: cerb_host_pack_stem
int cerb_devfwd_stem(const unsigned char* tiles, const float* tiles_f32, const float* w_raw, const float* scale, const float* shift, int host_pack, float* out, int N,
                     int H, int W, int relu, void* st) {
    DEV_NEED((tiles != nullptr) != (tiles_f32 != nullptr) && w_raw && scale && shift && out && N > 0 && H > 0 && W > 0);
    const hipStream_t s = (hipStream_t)st;
    float *dw = nullptr, *db = nullptr;
    hipError_t e = hipSuccess;
    if (host_pack) {
        std::vector<float> raw(64 * 147), wp;
        DEV_NEED(hipMemcpy(raw.data(), w_raw, raw.size() * 4, hipMemcpyDeviceToHost) == hipSuccess);
        cerb_host_pack_stem(raw.data(), scale, &wp);
        DEV_NEED(devfwd_upload(wp, &dw) == 0);
    } else {
        for (int c = 0; c < 64; ++c) DEV_NEED(scale[c] == 1.f);
        DEV_NEED(hipMalloc((void**)&dw, 7 * 12 * 2 * 64 * 4) == hipSuccess);
        e = cerb_launch_pack_stem(w_raw, dw, s);
    }
    if (devfwd_upload(std::vector<float>(shift, shift + 64), &db) != 0) e = hipErrorOutOfMemory;
    StemParams p;
    memset(&p, 0, sizeof(p));
    p.tiles = tiles; p.tiles_f32 = tiles_f32; p.wpack = dw; p.bias = db; p.out = out; p.N = N; p.H = H; p.W = W; p.relu = relu;
    if (e == hipSuccess) e = cerb_launch_stem(p, s);
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
    (void)hipFree(dw);
    (void)hipFree(db);
    return (int)e;
}

// One head of cerb_devfwd_head.  HOST: w1 [96][64], b1 [96], scale / shift [96] (the folded BatchNorm), w2 [out_ch][96], b2 [out_ch]; everything from
// `logits` on is a DEVICE pointer or null, with the meaning of HeadParams (cerb_common.h).
struct DevHead {
    const float *w1, *b1, *scale, *shift, *w2, *b2;
    int out_ch, kind, crop_y0, crop_x0, out_h, out_w, roi, pad_;
    float* logits;
    float* out_inst;
    unsigned char* out_type_u8;
    long long* out_type_i64;
    const long long* tile_off;
    long long tile_stride, row_stride;
    unsigned int* absmax_bits;
};
// launcher: 0 cerb_launch_head (one head, NHWC features), 1 cerb_launch_head_group with w2_44 = 0, 2 the same with w2_44 = 1.  feat: [N][H][W][64] NHWC, or
// (feat_planar) a tile-planar tensor of cerb_devfwd_planar_elems(N, H, W, 64) floats.  The shape rules are cerb_net_create's.
int cerb_devfwd_head(int launcher, const float* feat, int feat_planar, int N, int H, int W, const DevHead* heads, int n_heads, void* st) {
    DEV_NEED(launcher >= 0 && launcher <= 2 && feat && heads && N > 0 && H > 0 && W > 0 && n_heads >= 1 && n_heads <= 8);
    DEV_NEED(launcher != 0 || (n_heads == 1 && !feat_planar));
    for (int i = 0; i < n_heads; ++i) {
        const DevHead& h = heads[i];
        DEV_NEED(h.w1 && h.b1 && h.scale && h.shift && h.w2 && h.b2 && h.out_ch >= 2 && h.out_ch <= 8 && (h.kind == 0 || h.kind == 1));
        DEV_NEED(h.kind == 1 || h.out_ch == 2 || h.out_ch == 3);
        DEV_NEED(h.crop_y0 >= 0 && h.crop_x0 >= 0 && h.out_h > 0 && h.out_w > 0 && h.crop_y0 + h.out_h <= H && h.crop_x0 + h.out_w <= W);
        DEV_NEED(!(h.roi && h.logits) && (h.kind == 0 ? h.out_inst != nullptr : (h.out_type_u8 || h.out_type_i64)));
    }
    const hipStream_t s = (hipStream_t)st;
    HeadParams hp[8];
    std::vector<float*> owned;
    hipError_t e = hipSuccess;
    for (int i = 0; i < n_heads && e == hipSuccess; ++i) {
        const DevHead& h = heads[i];
        std::vector<float> pk[5];
        cerb_host_pack_head(h.w1, h.b1, h.scale, h.shift, h.w2, h.b2, h.out_ch, &pk[0], &pk[1], &pk[2], &pk[3], &pk[4]);
        float* d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        for (int k = 0; k < 5; ++k) {
            if (devfwd_upload(pk[k], &d[k]) != 0) e = hipErrorOutOfMemory;
            owned.push_back(d[k]);
        }
        HeadParams& p = hp[i];
        memset(&p, 0, sizeof(p));
        p.feat = feat; p.w1p = d[0]; p.b1 = d[1]; p.w2p = d[2]; p.b2 = d[3]; p.w2q = d[4];
        p.N = N; p.H = H; p.W = W; p.out_ch = h.out_ch; p.kind = h.kind;
        p.crop_y0 = h.crop_y0; p.crop_x0 = h.crop_x0; p.out_h = h.out_h; p.out_w = h.out_w; p.roi = h.roi;
        p.logits = h.logits; p.out_inst = h.out_inst; p.out_type_u8 = h.out_type_u8; p.out_type_i64 = h.out_type_i64;
        p.tile_off = h.tile_off; p.tile_stride = h.tile_stride; p.row_stride = h.row_stride; p.absmax_bits = h.absmax_bits;
        p.feat_planar = feat_planar;
        if (feat_planar) { p.pl_byp = cerb_planar_blocks(H); p.pl_bxp = cerb_planar_blocks(W); }
    }
    if (e == hipSuccess) e = launcher == 0 ? cerb_launch_head(hp[0], s) : cerb_launch_head_group(hp, n_heads, s, launcher == 2);
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
    for (float* q : owned) (void)hipFree(q);
    return (int)e;
}

// Patch-Class: x4 DEVICE [N][Hf][Wf][512]; HOST bn1 scale / shift [512], w1 [256][512], b1 [256], bn2 scale / shift [256], w2 [out_ch][256], b2 [out_ch];
// logits DEVICE [N][out_ch] or null; out DEVICE canvas or null, addressed like the heads'
int cerb_devfwd_patch_class(const float* x4, const float* bn1_scale, const float* bn1_shift, const float* w1, const float* b1, const float* bn2_scale,
                            const float* bn2_shift, const float* w2, const float* b2, int N, int Hf, int Wf, int out_ch, int out_h, int out_w, float* logits, float* out,
                            const long long* tile_off, long long tile_stride, long long row_stride, void* st) {
    DEV_NEED(x4 && bn1_scale && bn1_shift && w1 && b1 && bn2_scale && bn2_shift && w2 && b2 && N > 0 && Hf > 0 && Wf > 0 && out_ch >= 1 && out_ch <= 16);
    DEV_NEED((logits || out) && (!out || (out_h > 0 && out_w > 0)));
    const hipStream_t s = (hipStream_t)st;
    std::vector<float> pk[4];
    cerb_host_pack_patch_class(w1, b1, bn2_scale, bn2_shift, w2, b2, out_ch, &pk[0], &pk[1], &pk[2], &pk[3]);
    float* d[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 4; ++k)
        if (devfwd_upload(pk[k], &d[k]) != 0) e = hipErrorOutOfMemory;
    if (devfwd_upload(std::vector<float>(bn1_scale, bn1_scale + 512), &d[4]) != 0) e = hipErrorOutOfMemory;
    if (devfwd_upload(std::vector<float>(bn1_shift, bn1_shift + 512), &d[5]) != 0) e = hipErrorOutOfMemory;
    PatchClassParams p;
    memset(&p, 0, sizeof(p));
    p.x4 = x4; p.bn1_s = d[4]; p.bn1_b = d[5]; p.w1t = d[0]; p.b1 = d[1]; p.w2t = d[2]; p.b2 = d[3];
    p.N = N; p.Hf = Hf; p.Wf = Wf; p.out_ch = out_ch; p.out_h = out_h; p.out_w = out_w; p.logits = logits; p.out = out;
    p.tile_off = tile_off; p.tile_stride = tile_stride; p.row_stride = row_stride;
    if (e == hipSuccess) e = cerb_launch_patch_class(p, s);
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
    for (float* q : d) (void)hipFree(q);
    return (int)e;
}

// the decoder entry with a region of interest: roi = four HOST ints (y0, y1, x0, x1) in output pixels, or null
int cerb_devfwd_upsample2_add_roi(const float* skip, const float* prev, float* out, int G, int N, int H, int W, int C, long long prev_gs, const int* roi, void* st) {
    DEV_NEED(skip && prev && out && G > 0 && N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C % 4 == 0);
    DEV_NEED(!roi || (roi[0] >= 0 && roi[0] <= roi[1] && roi[1] <= H && roi[2] >= 0 && roi[2] <= roi[3] && roi[3] <= W));
    return (int)cerb_launch_upsample2_add(skip, prev, out, G, N, H, W, C, prev_gs, roi, (hipStream_t)st);
}
int cerb_devfwd_upsample2_add_planar_roi(const float* skip, const float* prev, float* out, int G, int N, int H, int W, int C, long long prev_gs, long long out_gs,
                                         const int* roi, int prev_planar, void* st) {
    DEV_NEED(skip && prev && out && G > 0 && N > 0 && H > 0 && W > 0 && out_gs >= cerb_planar_elems(N, H, W, C));
    DEV_NEED(!roi || (roi[0] >= 0 && roi[0] <= roi[1] && roi[1] <= H && roi[2] >= 0 && roi[2] <= roi[3] && roi[3] <= W));
    return (int)cerb_launch_upsample2_add_planar(skip, prev, out, G, N, H, W, C, prev_gs, out_gs, roi, prev_planar, (hipStream_t)st);
}

// ---- the fused output-head passes of the training step (head_train.hip; tests/test_head_train_parity_gpu.py), and the two separate passes they replaced --
int cerb_dev_head_train_supported(long long rows, int cin, int chid, int out) { return cerb_head_train_supported(rows, cin, chid, out) ? 1 : 0; }
// in_mean .. in_beta: the BatchNorm in front of the head, all four or none.  bn_part: [2048][96][2] doubles at most; *bn_blocks: rows of it written
int cerb_dev_head_fwd1(const float* prev, const float* w1, const float* b1, float* hid, long long rows, double* bn_part, int* bn_blocks, const float* in_mean,
                       const float* in_rstd, const float* in_gamma, const float* in_beta, void* st) {
    DEV_NEED(prev && w1 && b1 && hid && rows > 0);
    DEV_NEED((in_mean != nullptr) == (in_rstd != nullptr) && (in_mean != nullptr) == (in_gamma != nullptr) && (in_mean != nullptr) == (in_beta != nullptr));
    const float* in_bn[4] = {in_mean, in_rstd, in_gamma, in_beta};
    return (int)cerb_launch_head_fwd1(prev, w1, b1, hid, rows, bn_part, bn_blocks, (hipStream_t)st, in_mean ? in_bn : nullptr);
}
int cerb_dev_head_fwd2(const float* hid, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* w2, const float* b2, float* logits,
                       long long rows, int out, void* st) {
    DEV_NEED(hid && mean && rstd && gamma && beta && w2 && b2 && logits && rows > 0 && out > 0);
    return (int)cerb_launch_head_fwd2(hid, mean, rstd, gamma, beta, w2, b2, logits, rows, out, (hipStream_t)st);
}
size_t cerb_dev_head_bwd_workspace_bytes(long long rows, int out) { return rows > 0 && out > 0 ? cerb_head_bwd_workspace_bytes(rows, out) : 0; }
int cerb_dev_head_bwd1(const float* hid, const float* dlog, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* w2, float* dw2,
                       float* db2, float* dgamma, float* dbeta, long long rows, int out, void* ws, void* st) {
    DEV_NEED(hid && dlog && mean && rstd && gamma && beta && w2 && dw2 && db2 && dgamma && dbeta && ws && rows > 0 && rows % 16 == 0);
    return (int)cerb_launch_head_bwd1(hid, dlog, mean, rstd, gamma, beta, w2, dw2, db2, dgamma, dbeta, rows, out, ws, (hipStream_t)st);
}
// in_part: [min(rows / 64, cerb_head_bwd2_blocks())][64][2] doubles; *in_blocks (optional) reports that row count
int cerb_dev_head_bwd2(const float* hid, const float* dlog, const float* prev, const float* mean, const float* rstd, const float* gamma, const float* beta,
                       const float* dgamma, const float* dbeta, const float* w1, const float* w2, float* dprev, float* dw1, float* db1, long long rows, int out, int eval_mode,
                       int assign, void* ws, const float* in_mean, const float* in_rstd, const float* in_gamma, const float* in_beta, double* in_part, int* in_blocks,
                       void* st) {
    DEV_NEED(hid && dlog && prev && mean && rstd && gamma && beta && dgamma && dbeta && w1 && w2 && dprev && dw1 && db1 && ws && rows > 0);
    DEV_NEED((in_mean != nullptr) == (in_rstd != nullptr) && (in_mean != nullptr) == (in_gamma != nullptr) && (in_mean != nullptr) == (in_beta != nullptr));
    DEV_NEED(!in_part || in_mean);
    if (in_blocks) *in_blocks = (int)std::min<long long>(rows / 64, cerb_head_bwd2_blocks());
    const float* in_bn[4] = {in_mean, in_rstd, in_gamma, in_beta};
    return (int)cerb_launch_head_bwd2(hid, dlog, prev, mean, rstd, gamma, beta, dgamma, dbeta, w1, w2, dprev, dw1, db1, rows, out, eval_mode, assign, ws, (hipStream_t)st,
                                      in_mean ? in_bn : nullptr, in_part);
}
// in_scale: null or [rows][cin] (a dropout mask times 1 / (1 - p), per row and channel).  bn_part: [2048][cout][2] doubles at most, or null; *bn_blocks: rows of
// it written (0: the layer did not produce them)
int cerb_dev_pointwise(const float* in, const float* w, const float* bias, float* out, long long rows, int cin, int cout, const float* in_scale, double* bn_part,
                       int* bn_blocks, void* st) {
    DEV_NEED(in && w && bias && out && rows > 0 && cin > 0 && cout > 0);
    return (int)cerb_launch_pointwise(in, w, bias, out, rows, cin, cout, in_scale, (hipStream_t)st, bn_part, bn_blocks);
}
int cerb_dev_bn_apply(float* x, const float* src, const float* resid, long long group_stride, long long rows, int C, int groups, const float* mean, const float* rstd,
                      const float* gamma, const float* beta, int relu, void* st) {
    DEV_NEED(x && mean && rstd && gamma && beta && rows > 0 && C > 0 && groups > 0 && group_stride >= rows * C);
    return (int)cerb_launch_bn_apply(x, src, resid, group_stride, rows, C, groups, mean, rstd, gamma, beta, relu, (hipStream_t)st);
}

}  // extern "C"
