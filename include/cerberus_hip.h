/* cerberus_hip.h -- C ABI of libcerberus_hip.so: the MI355X (gfx950) tiled-inference hot path of Cerberus.
 *
 * This is the drop-in boundary.  The reference is pure Python; the objects this ABI
 * replaces are cited per entry point as <reference file>:<line>.  No torch types cross the boundary: plain
 * pointers (device pointers are raw hipMalloc/torch addresses), sizes, and a hipStream_t passed as void*.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure (CERB_ERR_ALLOC = 2 when a workspace allocation did not fit the
 *     device -- the one failure a caller can react to, e.g. with a smaller batch --, 1 otherwise); cerb_last_error() returns a thread-local
 *     message (the reference's only error convention is Python exceptions / assert, e.g.
 *     loader/postproc.py:390,395 and load_state_dict(strict=True) at infer/base.py:45).
 *   - one cerb_net per GPU / per process; calls on one handle must be serialised by the caller (the reference
 *     calls run_step from the main thread only, infer/tile.py:349-359).
 *   - the library owns packed weights and its workspace; the caller owns every input/output buffer.
 *   - activations are NHWC fp32; image tiles are NHWC uint8 (what infer_step receives, models/run_desc.py:439-441).
 */
#ifndef CERBERUS_HIP_H
#define CERBERUS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cerb_net cerb_net;
#define CERB_ERR_ALLOC 2

int cerb_version(void); /* 4: with the polygon fill (cerb_overlay_fill / _labels); 3: with the instance overlays (the cerb_overlay entries below); 2: with the training augmentations (cerb_aug); 1 before */
const char* cerb_last_error(void);

/* ---- network construction: replaces create_model / NetDesc.__init__ (models/net_desc.py:23-103,203) ----------
 * decoder_names[i]  e.g. "Lumen","Gland","Nuclei","Nuclei#TYPE","Gland#TYPE","Patch-Class"  (decoder_kwargs order,
 *                   already filtered by considered_tasks, models/net_desc.py:61-63)
 * head_names[i]     "INST" | "TYPE" | "OUT"        (an output head of that decoder)
 * out_ch[i]         number of output channels of that head (3,3,3,7,3,9 in models/paramset.yml:46-60).  An INST head has 3 (inner, contour: the
 *                   IP-ERODED-CONTOUR-* targets) or 2 (inner alone: the IP-ERODED-* targets) channels; TYPE heads 2..8; anything else is refused.
 * One entry per OUTPUT HEAD.  A decoder with several heads (models/net_desc.py:81-87: `{"Gland": {"INST": 3, "TYPE": 3}}` builds one decoder
 * trunk and a ModuleDict of heads over it, :196-198) is listed once per head, the decoder name repeated: the trunk's convolutions are loaded and
 * run ONCE, every head reads its features; out[] / logits[] of cerb_forward_io stay per entry.  (Inference only: a train-packed handle refuses it.)
 * Only encoder_backbone_name == "resnet34" exists in this library. */
int cerb_net_create(const char* const* decoder_names, const char* const* head_names, const int* out_ch,
                    int n_decoders, cerb_net** out_net);
void cerb_net_destroy(cerb_net* net);

/* ---- weights: replaces net.load_state_dict(saved_state_dict, strict=True) (infer/base.py:28-45) ----------------
 * One call per state-dict entry, using the reference's key names (backbone.layer1.0.conv1.weight, ...).  `data`
 * is a HOST pointer to contiguous fp32 in PyTorch's layout (conv: [Cout][Cin][kh][kw]); the library copies it.
 * Keys with integer payloads (num_batches_tracked) and the unused backbone.fc.* are accepted and ignored.
 * cerb_net_finalize folds eval-mode BatchNorm into the convolutions, packs for the MFMA kernels, uploads, and
 * fails (strict) if any required key is missing or has the wrong shape. */
int cerb_net_load_tensor(cerb_net* net, const char* key, const float* data, const int64_t* shape, int ndim);
int cerb_net_finalize(cerb_net* net);

/* ---- forward + output wrapper: replaces infer_step (models/run_desc.py:439-502) incl. NetDesc.forward
 * (models/net_desc.py:144-200), softmax / channel slice / centre crop / argmax, and -- through tile_off /
 * row_stride -- the stitching of infer/tile.py:141-163 (outputs can be written straight into a slide canvas).
 *
 * For decoder i (same order as cerb_net_create):
 *   INST head : out[i] -> float  [..][out_ch-1]  softmax channels 1..out_ch-1: [2] for a 3-class head, [1] for a 2-class one (run_desc.py:452-455);
 *               the destination's pixel stride follows the head, the addressing below stays in pixels
 *   TYPE head : out[i] -> int64 or uint8 class id (argmax of softmax)   (run_desc.py:490-491), see type_is_u8
 *   OUT  head : out[i] -> float class id broadcast over out_h x out_w   (Patch-Class, run_desc.py:480-487)
 * Destination addressing (in pixels): tile n, row y, col x  ->  (tile_off ? tile_off[n] : n*tile_stride)
 *                                                               + y*row_stride + x
 * logits[i] (optional, may be NULL) receives the raw head logits NHWC [N][H][W][out_ch] ([N][out_ch] for OUT). */
typedef struct cerb_forward_io {
    const uint8_t* tiles;      /* device, [N][H][W][3] uint8 RGB */
    int n, h, w;               /* batch, tile height/width (multiples of 16) */
    int out_h, out_w;          /* centre-crop size (cropping_center, misc/utils.py:94-104) */
    void* const* out;          /* [n_decoders] device pointers (NULL = head not wanted) */
    float* const* logits;      /* optional [n_decoders] device pointers or NULL */
    const long long* tile_off; /* optional device array [N] of pixel offsets into the destination */
    long long tile_stride;     /* used when tile_off == NULL; 0 means out_h*out_w */
    long long row_stride;      /* 0 means out_w */
    int type_is_u8;            /* 0: TYPE heads write int64 (reference dtype); 1: uint8 (device-resident canvas) */
    float* const* feats;       /* optional [6]: x0,x1,x2,x3,conv_map(x4),x4 NHWC dumps for tests, or NULL */
    const float* tiles_f32;    /* used when tiles == NULL: device [N][H][W][3] float pixel values (any floats; divided by 255 in fp32 like
                                * `imgs / 255.0`, models/net_desc.py:147) -- NetDesc.forward on inputs that are not whole numbers in 0..255 */
    unsigned int* logit_absmax; /* optional device uint32 [n_decoders] or NULL: the data-aware precision guard.  The head kernels raise word i
                                * (atomic max) to the IEEE-754 bit pattern of the largest |logit| of dense head i over every pixel this forward
                                * evaluates (non-negative floats order like their bits) -- the caller zeroes it when it wants a fresh maximum and
                                * reads it back as float.  Words of heads that were not requested, and of the OUT head, are left alone.  The
                                * F(4x4,3x3) default of cerb_net_set_conv_algo holds the 1e-4 contract while a model's logits stay in the range
                                * the parity fixtures cover; this is how a caller watches REAL data for batches that leave it
                                * (cerberus_amd/wsi.py counts them and can re-run them on conv_algo 1). */
} cerb_forward_io;

int cerb_net_forward(cerb_net* net, const cerb_forward_io* io, void* hip_stream);

/* Algorithm of the 3x3 stride-1 convolutions (90 % of the FLOPs), all on the exact-fp32 matrix instructions unless stated:
 *   6 (default) = Winograd F(4x4,3x3) for maps of 16 x 16 pixels and more -- conv_wino4b.hip up to 64 x 64, conv_wino4.hip above --
 *                 and F(2x2,3x3) below; the choice looks at the layer's geometry only, never at the batch size or the region of
 *                 interest, so a tile's values do not depend on what it is batched with;
 *   5, 7        = F(4x4,3x3) everywhere, with conv_wino4.hip / conv_wino4b.hip (36 products per 4x4 outputs instead of 144; transform
 *                 points 0, +-1, +-2, inf; probability maps within 4e-6 of the fp64 evaluation, tests/tools/dev_wino4_numerics.py);
 *   1           = Winograd F(2x2,3x3) (conv_wino.hip, round 1's default; same fp32 products, 2.25x fewer multiplies than direct);
 *   0           = direct implicit GEMM (conv_igemm.hip).
 * cuDNN makes the same kind of choice per layer for the reference (torch.backends.cudnn, models/run_desc.py:447).  All meet the 1e-4
 * bar; the switch exists for A/B measurement and for the parity tests of each path.
 * (Three F(2x2) variants that lost their A/B -- bf16x3-split products and two other work decompositions -- live in scripts/experiments/,
 * outside the product library.)
 * The training step follows the same rule for its forward and data-gradient convolutions (filter transform on the device). */
int cerb_net_set_conv_algo(cerb_net* net, int algo);
/* Layout of the private tensors (skip + upsample, first conv output, level output / head features; models/net_desc.py:182-198) of the
 * decoder levels: the last level and the level below it (both 64 channels; a level takes part when its maps are at least 64 x 64 pixels) and,
 * when both do, the two lowest levels (maps of at least one 16 x 16 block with sides that are multiples of 4; a level only if the one above it):
 *   1 (default) = tile-planar (cerb_common.h: cerb_planar_offset) through upsample2_add_planar -> conv_wino4p.hip x2 -> heads: a Winograd
 *                 wave's stores are contiguous 1-KiB rows and its patch loads whole lines, zero padding is data;
 *   0           = NHWC through conv_wino4.hip / conv_wino4b.hip (round 2's path).
 * Same arithmetic in the same order: the outputs are bit-identical (tests/test_net_gpu.py, tests/test_decoder_low_planar_gpu.py).  Applies with conv_algo 6 and head_algo 1. */
int cerb_net_set_planar(cerb_net* net, int enable);
/* Work items of the F(4x4,3x3) kernel for maps up to 64 x 64 pixels (conv_wino4b.hip) on maps whose sides are multiples of 4 but not of 16 -- the
 * 28 x 28 / 56 x 56 maps of the reference's default 448-pixel patch (infer/tile.py:43-106, models/backbone/resnet.py:273-286), in inference and in
 * the training step's forward and data-gradient convolutions:
 *   1 (default) = an item is 16 CONSECUTIVE 4x4 tiles of the batch (image-major, row-major): no padding tiles but in the launch's last item;
 *   0           = an item is a 16 x 16-pixel block (28 x 28 -> 2 x 2 blocks per image, 23 % of them padding).
 * A tile's arithmetic does not depend on the item it rides in: the outputs are bit-identical (tests/test_net_gpu.py).  For A/B. */
int cerb_net_set_packed_items(cerb_net* net, int enable);
/* Output heads (models/utils/net_layers.py:31-38): 1 (default) = every dense head of the batch in ONE grouped launch with the head's
 * weights resident in LDS (head_group_kernel) and the 96 -> 3 / 7 logits on 4x4x1 matrix instructions (no zero-padded rows); 2 = round 3's
 * grouped launch (logits on a 16-row instruction, 13 / 9 rows of zeros); 0 = one launch per head (round-1 head_kernel).  0 and 2 are
 * bit-identical to each other; 1 sums the 96 products of a logit in another order (a few 1e-7 on the logits).  For A/B. */
int cerb_net_set_head_algo(cerb_net* net, int algo);
/* Centre-crop regions of interest (default 1 = on).  infer_step keeps only the centre out_h x out_w window of every head
 * (models/run_desc.py:452-491 cropping_center; the reference's default geometry 448 -> 144 keeps 10 % of the pixels it computes).
 * With the switch on (any Winograd algorithm), every decoder level computes only the part of its maps that the kept window depends on
 * (3x3 conv: +1 pixel per layer, then out to whole 4x4 Winograd tiles; bilinear x2: +1 source pixel) and the heads only the window; the encoder still sees the whole
 * tile.  Results inside the window are bit-identical to the full computation (tests/test_net_gpu.py).  Ignored (full
 * computation) when full-size logits are requested or out == in. */
int cerb_net_set_crop_roi(cerb_net* net, int enable);

/* FLOPs (2*MAC) of one forward for the given geometry -- used by bench.py for the roofline figure. */
double cerb_net_flops(const cerb_net* net, int n, int h, int w);

/* Bytes of activation workspace the handles of this process hold right now (they grow with the largest batch run and stay until the handle is
 * destroyed).  A caller that prices its next job against the FREE device memory -- cerberus_amd/stream_bands.py::plan_slide, the counterpart of the
 * reference's chunk / tile sizing in infer/wsi.py:551-556 -- adds them back: they are allocated already and part of what a forward needs. */
size_t cerb_device_bytes_held(void);

/* Per-launch timing of the NEXT forwards with HIP events on the caller's stream (bench.py roofline leg; adds two
 * event records per kernel, so never enabled inside a timed region).  After a forward + stream sync,
 * cerb_net_profile_get(i) returns layer name, kernel family, algorithmic FLOPs and elapsed ms of launch i. */
int cerb_net_profile_enable(cerb_net* net, int enable);
int cerb_net_profile_count(cerb_net* net);
int cerb_net_profile_get(cerb_net* net, int idx, char* name, int name_cap, char* kernel, int kernel_cap, double* flops,
                         float* ms);

/* ---- post-processing: replaces PostProcInstErodedContourMap.post_process (loader/postproc.py:268-407) -----------
 * inst : device float [H][W][2] (ch0 = inner, ch1 = contour), `pix_stride` floats between consecutive pixels
 *        (2 for a packed INST map) and `row_stride` floats between rows -- lets it read a canvas window in place.
 * labels_out : device int32 [H][W]; ids as the reference assigns them (raster order of first pixel).
 * n_inst_out : device int32[1]; number of instances (nuclei: number of watershed markers; -1 when the map has no
 *        foreground at all, the branch in which the reference returns an all-zero float64 map, postproc.py:379-380).
 *        n_ambiguous_out : device int32[1] (nuclei only): number of watershed regions whose result depends on the order
 *        in which skimage's global binary heap releases marker pixels of bit-identical priority
 *        (skimage.segmentation.watershed, loader/postproc.py:378; DESIGN.md "watershed ties").  0: the parallel floods'
 *        label map is provably what skimage produces.  > 0: with exact_ties != 0 the map has been
 *        re-flooded on the device by a literal replay of that heap and is skimage's result as well; with exact_ties == 0 those regions
 *        keep the raster-order tie break.
 * ws / ws_bytes : caller-allocated device workspace of at least cerb_pp_workspace_bytes(H, W).
 * Streams: everything is ordered on `hip_stream`.  cerb_postproc_nuclei forks its independent flood tiers onto three internal
 * side streams per device (created on first use, joined back into `hip_stream` with events before it returns) -- the only
 * process-level state of the library; like the reference's run_step / post_process it is meant to be driven from one host
 * thread per GPU (SURVEY par.8b). */
size_t cerb_pp_workspace_bytes(int h, int w);
int cerb_postproc_nuclei(const float* inst, int h, int w, long long row_stride, int pix_stride, int32_t* labels_out,
                         int32_t* n_inst_out, int32_t* n_ambiguous_out, int exact_ties, void* ws, size_t ws_bytes, void* hip_stream);
int cerb_postproc_gland(const float* inst, int h, int w, long long row_stride, int pix_stride, float ds_factor,
                        int32_t* labels_out, int32_t* n_inst_out, void* ws, size_t ws_bytes, void* hip_stream);
int cerb_postproc_lumen(const float* inst, int h, int w, long long row_stride, int pix_stride, float ds_factor,
                        int32_t* labels_out, int32_t* n_inst_out, void* ws, size_t ws_bytes, void* hip_stream);
/* PostProcInstErodedMap.post_process (loader/postproc.py:147-265; the IP-ERODED-3 / -11 codes of infer/tile.py:35-40) for a two-class INST head.
 * inner : device float, ONE probability per pixel (`pix_stride` 1 for a packed map), row_stride / labels_out / n_inst_out / ws as above.
 * tissue: 0 Gland, 1 Lumen, 2 Nuclei.  fg = inner > 0.5; remove_small_objects(min_size 1500 / 150 / 8); 4-connected labels in raster order; per id
 * ascending: bounding box padded by 2 * ksize (ksize 11 / 3 / 3) on each side only where the padded edge stays inside, dilation by the ksize x ksize
 * ellipse inside that crop, holes filled inside that crop, pasted (later ids overwrite).  Nuclei take this scheme too -- no watershed.  There is no
 * ds_factor: the reference's `scale` argument is never read.  A map without a single background pixel comes back empty, as in the reference (its id list
 * `np.unique(inst_lab)[1:]` drops the smallest label, which is then the one instance). */
int cerb_postproc_eroded(const float* inner, int h, int w, long long row_stride, int pix_stride, int tissue, int32_t* labels_out,
                         int32_t* n_inst_out, void* ws, size_t ws_bytes, void* hip_stream);
/* Lumen *= (Gland > 0)   (infer/tile.py:187-191, infer/wsi.py:799-804) */
int cerb_mask_lumen_by_gland(int32_t* lumen_labels, const int32_t* gland_labels, long long n_pix, void* hip_stream);

/* ---- the slide reader's reduction to the processing resolution, on the device ------------------------------------------
 * The reference reads every patch through tiatoolbox's read_bounds at `wsi_proc_mag` (infer/wsi.py:521-527, 936-950): for a 40x scan that is a
 * x2 reduction of level 0 done on its DataLoader workers.  Here the host only decodes the stored level's rows; these two apply the reduction
 * (cerberus_amd/reader.py::read_bounds is the host statement, and they return its bytes).
 *   src : uint8 RGB rows of the level's window, src_row_stride BYTES between rows, src_rows x src_cols pixels; dst likewise.
 *   cerb_resample_box : integer factor k, exact k x k means rounded half to even, source indices clamped to the window (edge replication).
 *   cerb_resample_area: area means on a global grid through per-axis tables (reader.area_tables): idx int32 [n_out][taps] source positions,
 *                       w float32 [n_out][taps], wsum float32 [n_out] (the divisor), rep int32 [n_out] (>= 0: repeat that source position);
 *                       rows first, then columns, float32 multiply / add / divide in the host's order, rint, clip. */
int cerb_resample_box(const uint8_t* src, long long src_row_stride, int src_rows, int src_cols, int k, uint8_t* dst,
                      long long dst_row_stride, int out_rows, int out_cols, void* hip_stream);
int cerb_resample_area(const uint8_t* src, long long src_row_stride, int src_rows, int src_cols, uint8_t* dst,
                       long long dst_row_stride, int out_rows, int out_cols, const int32_t* row_idx, const float* row_w,
                       const float* row_wsum, const int32_t* row_rep, int row_taps, const int32_t* col_idx, const float* col_w,
                       const float* col_wsum, const int32_t* col_rep, int col_taps, void* hip_stream);

/* ---- slide-level data movement (device-resident slide; replaces the DataLoader side of the hot loop) ------------
 * cerb_synth_slide    : synthetic RGB slab [h][w][3]; pixel value depends only on (seed, y0+y, x0+x) so every sharding
 *                       of a slide sees the same pixels (BASELINE.json configs[2..3] "synthetic WSI").
 * cerb_gather_patches : tiles[k] = win x win window with top-left (tl_y[k], tl_x[k]) in ABSOLUTE slide coordinates,
 *                       mirror-padded outside the slide like np.pad(..., "reflect") (infer/tile.py:69); `slide` holds
 *                       rows [slide_y0, slide_y0+h) of a slide that is full_h rows tall (a rank's band + halo).
 *                       Replaces loader/infer_loader.py:54-69 / infer/wsi.py:936-950 for a resident slide.
 * cerb_downsample2_inst: dst[cerb_half_size(h)][cerb_half_size(w)][2] = cv2.resize(src, (0,0), fx=0.5, fy=0.5, INTER_LINEAR)
 *                       of an INST map (infer/wsi.py:786-788): the 2x2 box average, and for an odd side whose half rounds up
 *                       (cvRound, half to even) the last row / column replicated.
 * cerb_downsample2_inst_region: the same after multiplying the map by one tissue region of the slide mask
 *                       (infer/wsi.py:742-776): region_lab = int32 label map of the mask (cerb_label_mask) cropped to the
 *                       region's bounding box [mh][mw], resized to [h][w] like cv2.resize(INTER_NEAREST); samples whose
 *                       mask label != region_id count as 0.  region_lab NULL = no mask.
 * cerb_downsample2_map / cerb_downsample2_map_region: the same two calls with the channel count as an argument: n_ch = 2 is
 *                       the call above, n_ch = 1 reads ONE float per source pixel (the map of a two-class INST head, codes
 *                       IP-ERODED-3 / -11) and writes dst[..][..][1]; plane c of an n_ch-channel call is bit-equal to plane c
 *                       of the two-channel call on the same data.  pix_stride >= n_ch.
 * cerb_pclass_tissue_map: dst[cvRound(h/4)][cvRound(w/4)] = cv2.resize(pclass, fx=fy=0.25, INTER_NEAREST) times the
 *                       INTER_NEAREST-resized slide mask (infer/wsi.py:688-716); mask NULL = all tissue.
 * cerb_label_mask     : 4-connected components of mask != 0, ids in raster order of first pixel (scipy.ndimage.label,
 *                       infer/wsi.py:724); ws as for cerb_postproc_*; n_out = device int32[1] number of regions. */
int cerb_synth_slide(uint8_t* out, long long h, long long w, long long y0, long long x0, uint32_t seed, void* hip_stream);
int cerb_gather_patches(const uint8_t* slide, long long h, long long w, long long slide_y0, long long full_h,
                        const long long* tl_y, const long long* tl_x, int n, int win, uint8_t* tiles, void* hip_stream);
int cerb_downsample2_inst(const float* src, long long row_stride, int pix_stride, int h, int w, float* dst,
                          void* hip_stream);
int cerb_half_size(int n);
int cerb_downsample2_inst_region(const float* src, long long row_stride, int pix_stride, int h, int w,
                                 const int32_t* region_lab, long long lab_row_stride, int mh, int mw, int region_id,
                                 float* dst, void* hip_stream);
int cerb_downsample2_map(const float* src, long long row_stride, int pix_stride, int h, int w, int n_ch, float* dst,
                         void* hip_stream);
int cerb_downsample2_map_region(const float* src, long long row_stride, int pix_stride, int h, int w, int n_ch,
                                const int32_t* region_lab, long long lab_row_stride, int mh, int mw, int region_id,
                                float* dst, void* hip_stream);
int cerb_pclass_tissue_map(const float* pclass, long long row_stride, int h, int w, const uint8_t* mask,
                           long long mask_row_stride, int mh, int mw, float* dst, void* hip_stream);
int cerb_label_mask(const uint8_t* mask, long long row_stride, int h, int w, int32_t* labels_out, int32_t* n_out,
                    void* ws, size_t ws_bytes, void* hip_stream);

/* ---- tissue mask of a slide thumbnail: misc/utils.py:195-244 (stain_entropy_otsu, morphology, get_tissue_mask) on the device ------------------
 * The reference's docstring promises a generated mask when none is supplied (infer/wsi.py:509); this is the routine behind that promise.  Every
 * call is ordered on hip_stream, allocates nothing and synchronises nothing; ws / ws_bytes: caller-owned device workspace of at least
 * cerb_tissue_workspace_bytes(h, w) bytes, 8-byte aligned.  h * w < 2^31.  Host arithmetic (the two tables, Otsu on 256 counts) is
 * cerberus_amd/tissue.py's.
 *   cerb_tissue_hed        misc/utils.py:198-199, (rgb2hed(img) * 255).astype(uint8): rgb uint8 [h][w][3] with row_stride bytes between rows ->
 *                          planes_out uint8 [3][h][w] (H, E, D).  lut: double [3][256][3] = [channel][value][stain], the per-channel logarithm times
 *                          the stain matrix; byte = trunc(((lut[0][r] + lut[1][g]) + lut[2][b]) * 255) modulo 256.
 *   cerb_tissue_entropy    misc/utils.py:203-208, rank.entropy(plane, disk(4)) of the three planes and (H + E) - D: ent_out double [h][w];
 *                          pixels outside the image are left out of the count; term_table: double [50][50], [pop][count] =
 *                          (count / pop) * log(count / pop) / log(2), summed in ascending bin order.  minmax_out: device double[2], the minimum and
 *                          maximum of ent_out (no floating-point atomics: per-block values folded by a second kernel).
 *   cerb_tissue_histogram  misc/utils.py:210, the histogram behind threshold_otsu: counts256_out int64[256] = np.histogram(ent, 256, (min, max))
 *                          by numpy's assignment rule against edges257 = np.linspace(min, max, 257) (device doubles).  Integer counts.
 *   cerb_tissue_threshold  misc/utils.py:211: mask_out uint8 [h][w] = ent > thr.
 *   cerb_tissue_morphology misc/utils.py:216-235: scipy binary_erosion by disk(3) (outside the image counts as clear), remove_small_holes(2000),
 *                          remove_small_objects(2000), scipy binary_dilation by disk(3), remove_small_holes(2000), binary_fill_holes; 4-connected.
 *                          mask_in / mask_out: uint8 [h][w], packed; out is 0 / 1. */
size_t cerb_tissue_workspace_bytes(int h, int w);
int cerb_tissue_hed(const uint8_t* rgb, long long row_stride, int h, int w, const double* lut, uint8_t* planes_out, void* hip_stream);
int cerb_tissue_entropy(const uint8_t* planes, int h, int w, const double* term_table, double* ent_out, double* minmax_out, void* ws,
                        size_t ws_bytes, void* hip_stream);
int cerb_tissue_histogram(const double* ent, int h, int w, const double* edges257, int64_t* counts256_out, void* hip_stream);
int cerb_tissue_threshold(const double* ent, int h, int w, double thr, uint8_t* mask_out, void* hip_stream);
int cerb_tissue_morphology(const uint8_t* mask_in, int h, int w, uint8_t* mask_out, void* ws, size_t ws_bytes, void* hip_stream);

/* ---- instance table: the segmented reductions of get_inst_info_dict (loader/postproc.py:12-75) on the device --------
 * labels: int32 label map (row stride in elements); type_map: optional uint8 class map (NULL = none).
 * table : device int64 [n_inst][16], row id-1 = {area, sum_x, sum_y, y1, y2 (exclusive), x1, x2 (exclusive), first,
 *         type_count[0..7]}, first = min(y*w + x) over the instance's pixels (its first pixel in raster order)  ->  box [[y1,x1],[y2,x2]], centroid (sum_x/area, sum_y/area) == cv2.moments m10/m00, m01/m00,
 *         majority type / type_prob.  Contour tracing (cv2.findContours) is not part of this entry point. */
int cerb_inst_table(const int32_t* labels, long long lab_row_stride, const uint8_t* type_map, long long type_row_stride,
                    int h, int w, int n_inst, long long* table, void* hip_stream);

/* Outer border of every instance = cv2.findContours(mask, RETR_TREE, CHAIN_APPROX_SIMPLE)[0][0] of loader/postproc.py:29-41
 * (Suzuki-Abe border following, 8-connected foreground, start at pixel table[i][7] -- `table` is cerb_inst_table's output,
 * whose column 7 is the instance's first pixel: right for an instance that is ONE 8-connected piece; for several pieces
 * overwrite the column with cerb_inst_contour_start's result -- first move downwards/counter-clockwise, a point is kept where
 * the chain code changes).  Two passes:
 *   cerb_inst_contour_count  -> counts[i]  = number of points of instance i+1 (0 for absent ids)
 *   cerb_inst_contour_points -> points[2*(offsets[i] + k)] = x, [.. + 1] = y of point k; offsets = exclusive scan of counts (int64).
 * cerb_inst_contour_start -> start[i] = y*w + x of the pixel whose border findContours returns FIRST: OpenCV lists top-level
 *   contours most-recently-found first, so [0][0] belongs to the 8-connected piece whose first pixel comes last in raster
 *   order (one union-find pass over the label map; ws >= cerb_inst_contour_start_workspace_bytes(h, w) = 4 bytes per pixel,
 *   8 for maps of 2^31 pixels and more -- a 0.5-mpp scan of 60000 x 50000 is one).  Not modelled: a piece lying inside a HOLE of another
 *   piece of the same id is not a top-level contour in RETR_TREE and would be skipped by OpenCV.
 * OpenCV is not installed in this image: restated from the published algorithm, not pinned against the library. */
size_t cerb_inst_contour_start_workspace_bytes(int h, int w);
int cerb_inst_contour_start(const int32_t* labels, long long lab_row_stride, int h, int w, int n_inst, long long* start,
                            void* ws, size_t ws_bytes, void* hip_stream);
int cerb_inst_contour_count(const int32_t* labels, long long lab_row_stride, int h, int w, int n_inst, const long long* table,
                            int32_t* counts, void* hip_stream);
int cerb_inst_contour_points(const int32_t* labels, long long lab_row_stride, int h, int w, int n_inst, const long long* table,
                             const long long* offsets, int32_t* points, void* hip_stream);

/* out[y][x] = map[labels[y][x]] with map[0] == 0; ids outside [0, n_map) become 0.  Turns band-local instance ids into
 * slide-global ones after the count exchange of the sharded post-processing (the reference only needs ids to be unique:
 * uuid4 at infer/wsi.py:265,831). */
int cerb_relabel(const int32_t* labels, long long lab_row_stride, const int32_t* map, int n_map, int h, int w, int32_t* out,
                 long long out_row_stride, void* hip_stream);

/* ---- device timing helper: HIP events on the given stream (bench.py; torch.cuda.Event only sees torch's stream) */
/* ---- train-mode forward (BASELINE.json configs[4], forward half; models/run_desc.py:79-86) ---------------------------------------
 * cerb_net_set_fold_bn(net, 0), called BEFORE cerb_net_finalize, packs the network for training: raw convolution weights, the
 * BatchNorm affine parameters kept apart.  Such a network only serves cerb_net_forward_train (and an inference-packed one only
 * cerb_net_forward).  cerb_net_forward_train runs the reference's forward in `model.train()` mode: every BatchNorm normalises with
 * the statistics of the batch (biased variance, eps 1e-5), dropout of the Patch-Class branch takes its keep mask from the caller.
 *   tiles         : device uint8 [n][h][w][3]
 *   dropout_scale : device float [n][512] = keep / (1 - 0.3) of nn.Dropout(p=0.3) (models/net_desc.py:70), or NULL (no dropout)
 *   logits        : per decoder (cerb_net_create order) a device float buffer or NULL: dense heads [n][h][w][out_ch] (NHWC, full
 *                   resolution), Patch-Class [n][out_ch]
 * cerb_net_forward_train is the forward half alone; cerb_net_train_grads (below) records the activations on a tape and runs the backward
 * pass and returns the batch statistics from which the Python train_step updates the running ones. */
typedef struct cerb_train_io {
    const uint8_t* tiles;
    int n, h, w;
    const float* dropout_scale;
    float* const* logits;
} cerb_train_io;
int cerb_net_set_fold_bn(cerb_net* net, int fold);
/* Frozen modules of the sub-typing fine-tune (models/net_desc.py:105-142 `_freeze_weight`, called by train_step, models/run_desc.py:83-84): the
 * BatchNorm with state-dict prefix `bn_prefix` (e.g. "backbone.layer1.0.bn1") of a train-packed, finalized network runs in EVAL mode from now on --
 * cerb_net_forward_train / cerb_net_train_grads normalise it with these running statistics (host float[channels] each, eps 1e-5) instead of the
 * batch's and publish no batch statistics for it.  NULL statistics put it back in training mode.  Which parameters an optimiser then skips is the
 * caller's business (cerberus_amd/train.py drops the gradients of the frozen modules). */
int cerb_net_set_bn_eval(cerb_net* net, const char* bn_prefix, const float* running_mean, const float* running_var, int channels);
/* After an optimiser step: drop the packed weights of a finalized handle (activation workspaces, the training tape and the mode stay), so
 * that cerb_net_load_tensor of EVERY tensor + cerb_net_finalize install the updated parameters (models/run_desc.py:165 optimizer.step()). */
int cerb_net_begin_reload(cerb_net* net);
/* The optimiser's step without a host round trip (handles packed for training): copies each listed state-dict tensor from `dev_src[i]`
 * (device, float32, state-dict layout) into the handle's own copies and re-packs the conv weights with device kernels on `hip_stream`.
 * Keys the train-mode device path does not read (running statistics, num_batches_tracked, backbone.fc.*) are accepted and ignored. */
int cerb_net_update_params(cerb_net* net, int count, const char* const* keys, const float* const* dev_src, void* hip_stream);
int cerb_net_forward_train(cerb_net* net, const cerb_train_io* io, void* hip_stream);

/* cerb_net_train_grads: train-mode forward + the head losses + the backward pass of one step (models/run_desc.py:79-170 up to
 * all_loss.backward()), for a network packed with cerb_net_set_fold_bn(net, 0).  Weight gradients, the 3x3 data gradients and
 * the heads' pointwise layers run on the matrix cores, every reduction adds its partials in a fixed order (bitwise reproducible, no float
 * atomics).  Arrays are per decoder in
 * cerb_net_create order; a decoder whose target pointer is NULL contributes no loss.
 *   target[d]       : device float [n][h][w] class ids (Patch-Class: [n])          has_target[d] : device float [n]
 *   class_weight[d] : device float [out_ch] or NULL (see cerb_head_loss)           ce_w / dice_w / head_w : host floats
 *   loss_out        : device float [n_decoders], the value train_step reports per head (0 where no target was given)
 *   logits          : optional, as in cerb_train_io
 * Gradients are then read per state-dict key with cerb_net_grad_lookup (device pointer valid until the next call). */
typedef struct cerb_train_step_io {
    const uint8_t* tiles;
    int n, h, w;
    const float* dropout_scale;
    const float* const* target;
    const float* const* has_target;
    const float* const* class_weight;
    const float* ce_w;
    const float* dice_w;
    const float* head_w;
    float* loss_out;
    float* const* logits;
    const int* decoder_trained;  /* host int per decoder or NULL (= all): 0 reproduces a decoder outside train_decoder_list, whose
                                    gradients stay inside each of its blocks (models/net_desc.py:182 + conv_layers.py:44-53) */
    const float* const* pixel_weight; /* NULL, or per decoder NULL / device float [n][h][w]: the head's "#WEIGHT-MAP" target
                                         (models/run_desc.py:111-117), see cerb_head_loss_wmap */
} cerb_train_step_io;
/* Streams: everything is ordered on `hip_stream` as the caller sees it.  Inside, the weight gradients of the convolutions are queued on a second stream that
 * the handle owns -- forked from `hip_stream` by an event when a layer's output gradient is final, joined back into `hip_stream` before the call returns -- so work
 * the caller queues on `hip_stream` afterwards (optimiser, all-reduce, the next step) sees every gradient complete.  Not capturable into a hipGraph with the side
 * stream on (the developers' build of the library, libcerberus_hip_dev.so, reads CERB_WGRAD_SIDE=0 to keep the call on `hip_stream` alone: same bits). */
int cerb_net_train_grads(cerb_net* net, const cerb_train_step_io* io, void* hip_stream);
int cerb_net_grad_lookup(cerb_net* net, const char* key, float** dev_ptr, long long* numel);
/* The same lookup also serves the batch statistics of every BatchNorm of the step under "<bn prefix>.batch_mean" and
 * "<bn prefix>.batch_var" (unbiased), from which the caller updates running_mean / running_var (momentum 0.1).
 * cerb_adam_step: torch.optim.Adam (no weight decay / amsgrad; models/opt.py:47-58) on one parameter tensor, in place; `step` counts from 1. */
int cerb_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long numel, float lr, float beta1,
                   float beta2, float eps, int step, void* hip_stream);
/* The same update over `count` tensors in ONE launch (host arrays of device pointers and element counts): the 307 parameter tensors of
 * the six-head network per step. */
int cerb_adam_step_multi(int count, float* const* param, const float* const* grad, float* const* exp_avg, float* const* exp_avg_sq,
                         const long long* numel, float lr, float beta1, float beta2, float eps, int step, void* hip_stream);
/* device-to-device copy on a stream (lets a host language without a HIP binding move a looked-up gradient into its own buffer) */
int cerb_copy_d2d(void* dst, const void* src, size_t bytes, void* hip_stream);

/* ---- training step: per-head losses (BASELINE.json configs[4]; the whole step is cerberus_amd/train.py::train_step) --------------
 * cerb_head_loss: the per-head loss of the reference's train_step (models/run_desc.py:88-170) and its gradient on the logits.
 *   logits / dlogits : device float, element strides (n, c, y, x) -- NCHW as the reference's forward returns them, or NHWC
 *   target           : device float [N][H][W] class ids (the reference keeps targets in float32, :57-62)
 *   has_target       : device float [N], 1 where the sample carries this head's annotation (dummy_target protocol, :96-97)
 *   class_weight     : device float [C] or NULL.  Given (TYPE heads): pixel weight = class_weight[target], 0 on background
 *                      (get_class_wmap, :18-22,118-124) and the Dice term is masked by target > 0
 *   ce_weight, dice_weight, head_weight : paramset.yml loss_info ("ce" / "dice" weights inside the head, the head's own weight)
 *   patch_class_mode : 1 for the [N][C][1][1] Patch-Class head, which inherits the reference's [N] x [N,1,1] broadcast (:126-154)
 *   loss_out         : device float[1], the value train_step reports for the head; dlogits may be NULL (value only)
 *   ws               : device workspace of cerb_head_loss_workspace_bytes(N, H, W)
 * Sums are taken in a fixed order (per-block partials, one-block double-precision finalise): bitwise reproducible. */
size_t cerb_head_loss_workspace_bytes(int n, int h, int w);
int cerb_head_loss(const float* logits, long long stride_n, long long stride_c, long long stride_y, long long stride_x,
                   const float* target, const float* has_target, int n, int h, int w, int c, const float* class_weight,
                   float ce_weight, float dice_weight, float head_weight, int patch_class_mode, float* loss_out,
                   float* dlogits, void* ws, size_t ws_bytes, void* hip_stream);

/* The same with the head's per-pixel weight map (loader/targets.py "#WEIGHT-MAP" channel; models/run_desc.py:111-117,150): the pixel's
 * cross-entropy is multiplied by pixel_weight[n][y][x] (device float [N][H][W] or NULL = ones).  As in the reference, class weights
 * (TYPE heads) REPLACE the map, and the Patch-Class head has none. */
int cerb_head_loss_wmap(const float* logits, long long stride_n, long long stride_c, long long stride_y, long long stride_x,
                        const float* target, const float* has_target, int n, int h, int w, int c, const float* class_weight,
                        const float* pixel_weight, float ce_weight, float dice_weight, float head_weight, int patch_class_mode,
                        float* loss_out, float* dlogits, void* ws, size_t ws_bytes, void* hip_stream);

/* ---- training targets on the device: gen_targets (loader/targets.py:185-244) with fix_mirror_padding (loader/augs.py:7-21) --------------
 * ann: device int32 [n][h][w][c] instance / class annotations (what the reference's dataset hands gen_targets, batched).  A call handles up to
 * CERB_TARGET_MAX_HEADS heads of ONE kind over all n samples in batched launches; head i reads channel chan[i].  Outputs are [heads][n][crop_h]
 * [crop_w], centre-cropped with the reference's offset int((h - crop_h) * 0.5) (misc/utils.py:94-99).
 * cerb_target_pixel_maps : IP / NP (flag[i] = 1: binarise, loader/targets.py:61-65,169-175) and TP / PC (flag[i] = 0: pass through, :160-166,178-182).
 * cerb_target_eroded_maps: IP-ERODED-k (flag[i] = 0: inner map 0 / 1) and IP-ERODED-CONTOUR-k (flag[i] = 1: inner + 2 * contour), ksize[i] = k
 *                          (odd, 3..11; OpenCV's MORPH_ELLIPSE row spans, cerb_target_element).  Instances are the 4-connected components of equal
 *                          non-zero id (fix_mirror_padding's partition); only those with a pixel inside the crop count (:77-79,121-123); out-of-image
 *                          taps are ignored by erode and dilate.  meta != NULL: also labels the inner maps (scipy.ndimage.label's partition, :90,139)
 *                          for cerb_target_weight_maps and leaves in meta (device int32 [2 + heads * n]) the summed area of the labels' windows
 *                          (meta[0..1], one 64-bit count) and per image e = head * n_samples + sample its number of labels (meta[2 + e]).
 *                          ws: cerb_target_workspace_bytes(heads * n, h, w) bytes (25 B per pixel), kept untouched until cerb_target_weight_maps ran.
 * cerb_target_weight_maps: unet_weight_map (:12-58) + 1 for the maps cerb_target_eroded_maps labelled into ws: per label the exact Euclidean
 *                          distance inside its bounding box grown by 10 pixels (1000 outside), the two smallest over labels, w = 1 + 10 exp(-((d1 + d2)
 *                          / k)^2 / 2), 1 on labels and in maps with fewer than two labels.  max_labels >= every meta[2 + e], total_area = the 64-bit
 *                          meta[0..1]; win_ws: cerb_target_window_workspace_bytes(heads * n, max_labels, total_area) bytes.  dsum_out (optional):
 *                          d1 + d2 in float32 before the exponential (2000 in maps with fewer than two labels).  Squared distances are integers and
 *                          the reduction is a gather per pixel: results are bitwise reproducible.
 * cerb_target_element    : the k x k MORPH_ELLIPSE element (host bytes, 0 / 1) the morphology uses. */
#define CERB_TARGET_MAX_HEADS 8
typedef struct cerb_target_heads {
    int n_heads;
    int chan[CERB_TARGET_MAX_HEADS];
    int ksize[CERB_TARGET_MAX_HEADS];
    int flag[CERB_TARGET_MAX_HEADS];
} cerb_target_heads;
size_t cerb_target_workspace_bytes(int n_images, int h, int w);
size_t cerb_target_window_workspace_bytes(int n_images, int max_labels, unsigned long long total_area);
int cerb_target_element(int ksize, uint8_t* out);
int cerb_target_pixel_maps(const int32_t* ann, int n, int h, int w, int c, const cerb_target_heads* heads, int crop_h, int crop_w,
                           int32_t* out, void* hip_stream);
int cerb_target_eroded_maps(const int32_t* ann, int n, int h, int w, int c, const cerb_target_heads* heads, int crop_h, int crop_w,
                            int32_t* cls_out, int32_t* meta, void* ws, size_t ws_bytes, void* hip_stream);
int cerb_target_weight_maps(int n, int h, int w, const cerb_target_heads* heads, int crop_h, int crop_w, const void* ws, size_t ws_bytes,
                            int max_labels, unsigned long long total_area, void* win_ws, size_t win_ws_bytes, float* wmap_out,
                            float* dsum_out, void* hip_stream);

/* ---- validation statistics on the device: ProcStepRawOutput (models/run_desc.py:606-747) over valid_step's read-outs (:332-436) ------------
 * One grouped launch per step accumulates, per head and class, over_inter / over_total / over_correct / nr_pixels into a persistent device
 * accumulator acc: int64 [n_heads][CERB_VALID_MAX_CLASSES][4] in that order (cerb_valid_stats_bytes(n_heads) bytes; rows of classes a head does
 * not count stay 0).  flags: device bytes [n_heads][n], flags[head][sample] != 0 when the head's name appears anywhere in the sample's
 * dummy_target row (:642); only flagged samples count.  Per flagged sample, with p the prediction and t the true map, both [n][h][w]:
 *   CERB_VALID_INST  (:646-660) classes k = 1 .. C-1: pred_ = (p[..., k-1] > 0.5) * k; inter = #(pred_ == k and t == k), total = #(pred_ == k) +
 *                    #(t == k), correct = #(t == pred_) -- background agreeing with 0 included.  p: float32 [n][h][w][C-1] (softmax channels 1:).
 *   CERB_VALID_TYPE  (:661-674) classes k = 1 .. C-1: inter and total as above on p == k, counted only where t > 0; correct = #(t == p) without the
 *                    mask, the same number for every class.  p: class ids, uint8 (pred_fmt 0) or int64 (pred_fmt 1) [n][h][w].
 *   CERB_VALID_PATCH (:675-686) classes k = 0 .. C-1: as TYPE without the mask.  p: float32 class ids, the tile-broadcast map [n][h][w] (pred_fmt 0)
 *                    or one value per sample [n] (pred_fmt 1).
 *   every head       nr_pixels += h * w (:633,641).
 * t: int32 (true_fmt bit 0 clear) or float32 (bit 0 set) [n][h][w]; Patch-Class may give one value per sample [n] (bit 1 set).  Class ids are
 * compared as float32 (numpy's comparison of the reference's float32 maps); int32 ids must stay below 2^24 in magnitude.  NaN compares false.
 * The reference defines these statistics only for batches without a Patch-Class target (with one, its valid_step hands back [n][h][h][w] true
 * arrays that cannot be compared, and the callback raises); here the same per-head rules run on the natural [n][h][w] maps in both cases.
 * Counts are integers: the accumulator is independent of the order of blocks and bitwise reproducible.  No host synchronisation, no allocation;
 * the launch and cerb_valid_stats_reset (an asynchronous clear) run on hip_stream.  The summary (:526-561) is host arithmetic:
 * accuracy = (correct + 1e-8) / (nr_pixels + 1e-8), dice = 2 inter / (total + 1e-8), in float64 (cerberus_amd/valid_stats.py). */
#define CERB_VALID_MAX_HEADS 8
#define CERB_VALID_MAX_CLASSES 16
#define CERB_VALID_INST 0
#define CERB_VALID_TYPE 1
#define CERB_VALID_PATCH 2
typedef struct cerb_valid_heads {
    int n_heads;
    int kind[CERB_VALID_MAX_HEADS];
    int n_classes[CERB_VALID_MAX_HEADS];
    int pred_fmt[CERB_VALID_MAX_HEADS];
    int true_fmt[CERB_VALID_MAX_HEADS];
    const void* pred[CERB_VALID_MAX_HEADS];
    const void* true_map[CERB_VALID_MAX_HEADS];
} cerb_valid_heads;
size_t cerb_valid_stats_bytes(int n_heads);
int cerb_valid_stats_reset(int64_t* acc, int n_heads, void* hip_stream);
int cerb_valid_stats_accumulate(const cerb_valid_heads* heads, const uint8_t* flags, int n, int h, int w, int64_t* acc, void* hip_stream);

/* ---- JPEG tiles of a TIFF / .svs level: host Huffman pass, device IDCT / up-sampling / colour (cerberus_amd/jpeg_device.py) -------------------
 * Replaces, for compression-7 tiles, the per-tile PIL decode of the slide reader (cerberus_amd/reader.py: TiffReader._decode; the reference reads
 * slides through tiatoolbox's WSIReader on 12 DataLoader workers, infer/wsi.py:936-950) and returns ITS bytes.  The only serial part of a baseline JPEG
 * decode is the entropy decoder (csrc/jpeg_entropy.h, which states what is accepted, "unsupported" and "corrupt"); it runs on host threads and hands
 * QUANTISED coefficients over, everything after it runs in two kernels (csrc/jpeg_kernels.hip).
 *
 * Buffer layout ("stream buffer", the same bytes on the host and on the device): n_tiles tile headers (cerb_jpeg_hdr of jpeg_entropy.h, 464 bytes each:
 * status, size, sampling, colour decision, MCU grid, position in the level, coefficient offset, three de-zigzagged uint16 quantisation tables),
 * padded to a multiple of 256 bytes, then the int16 coefficients of the tiles that decoded, in natural order: per tile, per component, a raster of
 * (mcu_rows v) x (mcu_cols h) blocks of 64.
 *   cerb_jpeg_workspace_bytes(n_tiles, tile_w, tile_h, which): which = 0 the stream buffer for n_tiles tiles of that size whatever their sampling
 *                           (pinned host memory and its device copy); which = 1 the device scratch of cerb_jpeg_decode_window (the component planes).
 *   cerb_jpeg_decode_stream one stream (+ optional JPEGTables stream) -> header + coefficients; RETURNS THE STATUS: 0 decoded, 1 unsupported (not an
 *                           error), -1 corrupt, -2 the coefficients exceed coef_cap (int16 units).  No device involved.
 *   cerb_jpeg_read_tiles    HOST half of a window: pread of n_tiles byte ranges (offsets / counts) of fd and their entropy decode on up to n_threads
 *                           (<= 64) threads that take tiles off a shared counter, like cerb_host_tiff_read_tiles; the interpreter is not involved.  gx0 /
 *                           gy0: every tile's position in its level.  tables / n_tables: the page's JPEGTables (tag 347) or none.  photometric_rgb: the page's
 *                           PhotometricInterpretation is 2 (the components are R, G, B whatever the stream's markers say).  buf: 16-byte aligned, at least
 *                           cerb_jpeg_workspace_bytes(.., 0) bytes.  *used_bytes: the prefix of buf to copy to the device.  unsupported[0 .. *n_unsupported):
 *                           ascending indices of the tiles the caller must decode another way (also every stream whose size is not tile_w x tile_h); their
 *                           headers say so and the device half skips them.  A corrupt tile or a short read fails the call (1, cerb_last_error) with
 *                           *bad_tile = the first such index, else -1.
 *   cerb_jpeg_decode_window DEVICE half, two launches per 65535 tiles on hip_stream, no allocation, no synchronisation: dev_buf = the device copy of
 *                           the stream buffer's first dev_bytes bytes; scratch: 8-byte aligned, cerb_jpeg_workspace_bytes(.., 1) bytes; the part of every
 *                           decoded tile inside the window [x0, x1) x [y0, y1) of the level goes to dst + (y - y0) dst_row_stride + (x - x0) 3 (uint8 RGB).
 *                           Offsets in the headers are checked against dev_bytes / scratch_bytes; nothing outside the window is written.
 * Arithmetic (all integers, >> arithmetic, products in 64 bits), equal to PIL 12 / libjpeg-turbo bit for bit on what encoders write:
 *   dequantise c[k] q[k]; inverse DCT "islow" with 13-bit constants (2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172), pass 1 down
 *   the columns rounded to (x + 1024) >> 11, pass 2 along the rows (x + 131072) >> 18, sample = clamp(x + 128, 0, 255);
 *   chroma planes are cut to ceil(W / 2) (x ceil(H / 2)) BEFORE up-sampling.  4:2:2, per row: out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] =
 *   (3 in[i] + in[i+1] + 2) >> 2, the first and the last output copy their input.  4:2:0: s[i] = 3 in[r][i] + in[r'][i] with r' the nearer neighbour row
 *   (clamped), out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4 with i +- 1 clamped; then cropped to W x H;
 *   YCbCr -> RGB (cb, cr less 128): R = y + ((91881 cr + 32768) >> 16), G = y + ((-22554 cb - 46802 cr + 32768) >> 16), B = y + ((116130 cb + 32768)
 *   >> 16), clamped.  Outside the claim: libjpeg's range-limit table WRAPS samples more than about 384 beyond 0 .. 255 where this clamps, and its SIMD
 *   inverse DCT keeps 16-bit intermediates; only hostile streams (no encoder's output) get there. */
size_t cerb_jpeg_workspace_bytes(int n_tiles, int tile_w, int tile_h, int which);
int cerb_jpeg_decode_stream(const uint8_t* tables, long long n_tables, const uint8_t* src, long long n_src, int photometric_rgb, void* hdr,
                            int16_t* coefs, long long coef_cap, long long* coef_used);
int cerb_jpeg_read_tiles(int fd, int n_tiles, const int64_t* offsets, const int64_t* counts, const int32_t* gx0, const int32_t* gy0, int tile_w,
                         int tile_h, const uint8_t* tables, long long n_tables, int photometric_rgb, void* buf, size_t buf_bytes, int n_threads,
                         size_t* used_bytes, int32_t* bad_tile, int32_t* n_unsupported, int32_t* unsupported);
int cerb_jpeg_decode_window(const void* dev_buf, size_t dev_bytes, int n_tiles, int tile_w, int tile_h, uint8_t* scratch, size_t scratch_bytes,
                            uint8_t* dst, long long dst_row_stride, int x0, int y0, int x1, int y1, void* hip_stream);

/* ---- JPEG encoding of a picture on the device: colour / DCT / Huffman / packing (cerberus_amd/jpeg_encode.py) -----------------------------------
 * The mirror of "JPEG tiles" above: a uint8 RGB picture that lives on the device becomes the entropy-coded scan of a baseline JPEG file, and only the
 * compressed bytes cross to the host (csrc/jpeg_encode.hip; the headers around the scan are written in Python).  Not in the reference, which hands
 * whole pictures to cv2 / PIL on the host.  Equal to PIL's Image.save(format="JPEG", quality=q, subsampling=s) -- libjpeg's integer forward path, Annex-K
 * Huffman tables, optimize=False -- coefficient for coefficient, and to save(..., restart_marker_rows=1) byte for byte in the scan.
 *   cerb_jpeg_enc_workspace_bytes(w, h, subsampling, which): which = 0 the workspace of cerb_jpeg_enc_coefs (the component planes), 1 the bytes of the
 *                           coefficients, 2 the workspace of cerb_jpeg_enc_scan, 3 the most a scan of this picture can take (scan_cap that never
 *                           truncates).  0 for a size or a subsampling the calls refuse.
 *   cerb_jpeg_enc_coefs     src: uint8 RGB, rows row_stride bytes apart (>= 3 w; any alignment: a view into a larger picture is fine).  coefs: int16,
 *                           16-byte aligned, IN THE DECODER'S LAYOUT: per component a raster of (mcu_rows v) x (mcu_cols h) blocks of 64 in natural
 *                           order -- what cerb_jpeg_decode_window reads.  qtables: uint16 [2][64] on the device, the luminance and the chrominance
 *                           table in natural order, or null.  workspace: 8-byte aligned.  Two launches.
 *   cerb_jpeg_enc_scan      coefs -> scan_out[0 .. *scan_len_dev): every MCU row is one restart interval (DRI = MCU columns), RSTm (m = row mod 8)
 *                           between the intervals, none after the last.  workspace: 128-byte aligned.  *scan_len_dev (int64 on the device) is the
 *                           scan's full length; bytes at or past scan_cap are not written, so a caller that gave less than
 *                           cerb_jpeg_enc_workspace_bytes(.., 3) compares the two.  One memset and four launches.
 *   cerb_jpeg_enc_tiles     the coefficients of a w x h picture -> one abbreviated stream per tile x tile crop (the tiles of a JPEG-in-TIFF page;
 *                           cerberus_amd/tiff_pyramid.py).  w and h are multiples of tile, tile a multiple of 16 in 16 .. 512: the MCU grid, the 2 x 2
 *                           chroma boxes and the blocks then align with the tile grid, the crop's coefficients are a sub-raster of the picture's and
 *                           nothing is recomputed.  Tile i (row-major) becomes prefix[0 .. n_prefix) + the scan of the crop EXACTLY as
 *                           cerb_jpeg_enc_scan defines it for a tile x tile picture (an interval per MCU row of the tile, RSTm with m = the row
 *                           inside the tile mod 8, none after the last) + FF D9.  prefix: HOST bytes, n_prefix <= 64, copied into the launch
 *                           arguments (the caller's SOI SOF0 DRI SOS: 41 bytes).  offsets_dev: int64 [n_tiles + 1] on the device, offsets_dev[i]
 *                           the start of tile i in out -- always even, a zero byte follows a stream of odd length -- and offsets_dev[n_tiles] the
 *                           total; counts_dev: int64 [n_tiles], the unpadded lengths.  Bytes at or past out_cap are not written and the total is
 *                           reported all the same.  cerb_jpeg_enc_tiles_workspace_bytes(w, h, tile, subsampling, which): 0 the workspace (128-byte
 *                           aligned), 1 the out_cap that never truncates; 0 for arguments the call refuses.  Integer atomics only: the bytes do not
 *                           depend on the order of execution.  One memset and four launches; an interval has at most 192 blocks (one pass of a
 *                           workgroup).  Refuses before any launch, naming the argument: a bad tile, w or h no multiple of it, a workspace too small
 *                           or misaligned, a null pointer, n_prefix outside 0 .. 64.
 * All refuse BEFORE any launch (1, cerb_last_error names the argument): w or h outside 1 .. 32768, quality outside 1 .. 100, subsampling other than
 * 0 (4:4:4) / 2 (4:2:0), a workspace smaller than cerb_jpeg_enc_workspace_bytes says.  They queue on hip_stream, allocate nothing, do not synchronise.
 * Capacity: with the Annex-K tables a block takes at most 11 + 11 bits of DC and 63 x (16 + 10) bits of AC = 1660 bits < 208 bytes, so an interval of n
 * blocks has a slot of 208 n bytes (+ 8, rounded to 128) before stuffing and at most twice that + 2 in the scan: no 8-bit picture overruns at any
 * quality, and every store is checked against the slot / scan_cap all the same.
 * Arithmetic (all integers, >> arithmetic, products in 64 bits):
 *   colour  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
 *           Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16.
 *   edges   libjpeg's order: columns are replicated at FULL resolution out to the MCU grid (8 for 4:4:4, 16 for 4:2:0); rows are replicated at full
 *           resolution only up to an even count (4:2:0, odd h), the component is down-sampled, and ITS last row is replicated down to the MCU grid.
 *   4:2:0   out[r][c] = (p[2r][2c] + p[2r][2c+1] + p[2r+1][2c] + p[2r+1][2c+1] + bias) >> 2, bias 1 for even c and 2 for odd c.
 *   DCT     jfdctint ("islow") on sample - 128, the 13-bit constants of the inverse one.  Pass 1 along the rows: outputs 0 and 4 are (t10 +- t11) << 2,
 *           the others (x + 1024) >> 11.  Pass 2 down the columns: outputs 0 and 4 (x + 2) >> 2, the others (x + 16384) >> 15.  8 x the DCT.
 *   tables  Annex K scaled as libjpeg does: scale = 5000 / q (q < 50) else 200 - 2 q; entry = clamp((base scale + 50) / 100, 1, 255).
 *   quantisation  sign(c) ((|c| + (8 Q >> 1)) / (8 Q)).
 *   dummy blocks  4:2:0 only: a Y block of an MCU that lies wholly beyond Y's own grid of ceil(h / 8) x ceil(w / 8) blocks has no AC terms and the
 *           (quantised) DC of the block before it in the MCU's order; in a bottom row of dummies both blocks take the MCU's top-right block's.
 *   coding  baseline Huffman, Annex-K tables, zig-zag order, MCUs interleaved (4:2:0: four Y blocks in raster order, Cb, Cr); DC difference per
 *           component, predictors reset at every interval; category = bit length of |d|, magnitude bits d or d - 1 (d < 0); run / size symbols with ZRL
 *           for 16 zeros and EOB for a zero tail; every interval padded to a byte with 1-bits; FF followed by 00. */
size_t cerb_jpeg_enc_workspace_bytes(int w, int h, int subsampling, int which);
int cerb_jpeg_enc_coefs(const uint8_t* src, long long row_stride, int w, int h, int quality, int subsampling, int16_t* coefs, uint16_t* qtables,
                        void* workspace, size_t ws_bytes, void* hip_stream);
int cerb_jpeg_enc_scan(const int16_t* coefs, int w, int h, int subsampling, void* workspace, size_t ws_bytes, uint8_t* scan_out, size_t scan_cap,
                       long long* scan_len_dev, void* hip_stream);
size_t cerb_jpeg_enc_tiles_workspace_bytes(int w, int h, int tile, int subsampling, int which);
int cerb_jpeg_enc_tiles(const int16_t* coefs, int w, int h, int tile, int subsampling, const uint8_t* prefix, int n_prefix, void* workspace,
                        size_t ws_bytes, uint8_t* out, size_t out_cap, long long* offsets_dev, long long* counts_dev, void* hip_stream);

/* ---- instance metrics between two label maps: contingency table, PQ / AJI / Dice2 / Dice1 counters (cerberus_amd/inst_metrics.py) ------------------
 * Maps are int32 with a row stride in elements (every pixel offset is 64-bit: a view whose last row lies past 2^31 elements is fine); 0 is background
 * and an id outside [1, n_ids] -- negative, or above the bound the caller states -- counts as background too (as in cerb_relabel) and never indexes a
 * table.  Nothing outside h x w is read.  All calls queue on hip_stream, allocate nothing and do not synchronise.
 *   cerb_inst_areas        area[id] += pixels of id, for ids in [1, n_ids]; area: int64 [n_ids + 1], cleared by the caller (area[0] is not written).
 *   cerb_inst_pairs        the sparse table of pixel counts per (true id, pred id) with both > 0.  true_index / pred_index: int32 [n_ids + 1], the
 *                          1-based rank of every id that occurs among the ids that occur, 0 for one that does not (area > 0, exclusive scan); a
 *                          pair's key is (true rank << 32) | pred rank.  table: cerb_inst_pairs_workspace_bytes(capacity) bytes, 8-byte aligned,
 *                          capacity a power of two; the call clears it.  It starts with four int64 words {n_pairs, overflow, updates kept on chip,
 *                          updates sent to the table}, then keys[capacity] (0 = free) and counts[capacity].  Probing is bounded: when a key finds
 *                          no slot the update is DROPPED and overflow becomes 1 -- the result is then unusable and the caller repeats the call with a
 *                          larger capacity (4 x is what the Python side does).  Slots are taken modulo capacity: no overflow writes out of bounds.
 *   cerb_inst_pairs_compact  the occupied slots as keys_out / counts_out (int64, up to max_out entries, in no particular order -- sort by key);
 *                          *n_out (device int64, cleared by the call) = number of occupied slots.
 *   cerb_inst_pair_stats   from the pairs SORTED by key, the areas by rank (true_area[rank - 1]) and optional per-instance classes by rank:
 *                          summary (device int64 [CERB_INST_SUMMARY_WORDS]) = {tp, fp, fn, aji_inter, aji_union, dice2_inter, dice2_total,
 *                          dice1_inter, dice1_total, n_true, n_pred, 0} and *sum_iou (device double).  cls >= 0 keeps only the true and pred
 *                          instances of that class (both type vectors required) -- the same numbers as on maps with the other instances zeroed;
 *                          cls < 0: no filter.  ws: cerb_inst_pair_stats_workspace_bytes(n_true, n_pred) bytes, 8-byte aligned.
 * Rules, with a, b the areas, c > 0 a pair's count, u = a + b - c:
 *   a pair matches iff 2 c > u (IoU > 0.5; matches are unique); tp = matches, fn = n_true - tp, fp = n_pred - tp, sum_iou = sum of c / u over them.
 *   AJI: per true instance with a pair, the pred p* of largest c / u (compared as c1 u2 > c2 u1 in 128 bits; a tie goes to the smaller pred id):
 *   aji_inter += c, aji_union += u, p* is used; a true instance without a pair adds a to aji_union, every pred never used adds b.
 *   dice2_inter = sum c over the pairs, dice2_total = sum (a + b) over the pairs; dice1_inter = sum c, dice1_total = sum a + sum b over the instances.
 * Every decision is integer arithmetic.  sum_iou is float64, each term the correctly rounded c / u, added in one fixed order: two runs agree bitwise.
 * The ratios (dq, sq, pq, aji, dice2, dice1) are host arithmetic on these numbers (cerberus_amd/inst_metrics.py). */
#define CERB_INST_SUMMARY_WORDS 12
int cerb_inst_areas(const int32_t* labels, long long row_stride, int h, int w, int n_ids, long long* area, void* hip_stream);
size_t cerb_inst_pairs_workspace_bytes(long long capacity);
int cerb_inst_pairs(const int32_t* true_map, long long true_row_stride, const int32_t* pred_map, long long pred_row_stride, int h, int w,
                    const int32_t* true_index, int n_true_ids, const int32_t* pred_index, int n_pred_ids, void* table, long long capacity,
                    void* hip_stream);
int cerb_inst_pairs_compact(const void* table, long long capacity, long long* keys_out, long long* counts_out, long long max_out,
                            long long* n_out, void* hip_stream);
size_t cerb_inst_pair_stats_workspace_bytes(int n_true, int n_pred);
int cerb_inst_pair_stats(const long long* keys, const long long* counts, long long n_pairs, const long long* true_area, int n_true,
                         const long long* pred_area, int n_pred, const int32_t* true_type, const int32_t* pred_type, int cls,
                         long long* summary, double* sum_iou, void* ws, size_t ws_bytes, void* hip_stream);

/* ---- instance morphometry and relations between tissues (cerberus_amd/inst_features.py, csrc/inst_features.hip) ---------------------------------------
 * House rules of cerb_inst_*: maps are int32 with a row stride in elements and 64-bit pixel offsets; id 0 is background and so is any id outside
 * [1, n_inst] (negative or above the bound), which never indexes a table; nothing outside h x w is read; every call queues on hip_stream, allocates
 * nothing and does not synchronise.  `table` is cerb_inst_table's output for the SAME map and n_inst (int64 [n_inst][16]).
 *
 * cerb_inst_shape  shape: device int64 [n_inst][CERB_INST_SHAPE_WORDS], CLEARED by this call (all eight words), row id-1 =
 *       {m20, m02, m11, crack, border_px, hull_area2, hull_pts, rows}.  This call fills words 0..4; cerb_inst_hull_rows, called AFTER it, words 5..7.
 *     m20 = sum (x - x1)^2, m02 = sum (y - y1)^2, m11 = sum (x - x1)(y - y1) over the instance's pixels, (y1, x1) = the box corner table[.][3], [5]:
 *       raw second moments about the box corner.  Exact in int64 while every box side is < 2^16 and every area < 2^31 (each term < 2^32).
 *     crack = number of (pixel of the instance, one of its four neighbour directions) pairs whose neighbour lies outside the map or carries another
 *       id (background and out-of-range ids included; the neighbour is validated like the centre pixel): the 4-connected boundary length in pixel
 *       edges.  An edge between two touching instances counts for both.
 *     border_px = number of the instance's pixels with at least one such side.
 *     One lane per run of equal labels along a row inside a wave issues the atomics (3 for a run without a boundary side, 5 otherwise).
 *
 * cerb_inst_hull_rows  the convex hull of the instance's pixel CENTRES, in two passes behind one call.
 *     row_offsets: int64 [n_inst], the exclusive scan of the box heights max(y2 - y1, 0) (0 for an absent id).  extents: int32 [sum of box heights][2],
 *       cleared by the call to the empty sentinel {INT_MAX, INT_MIN}; pass 1 leaves {leftmost x, rightmost x} of the instance in every row of its box
 *       (a row without a pixel of the instance -- an instance of several pieces -- keeps the sentinel).  Pass 2 uses `extents` as its stacks: on
 *       return its content is unspecified.
 *     Pass 2, one thread per instance: the hull of a pixel set is the hull of its per-row extremes; a monotone chain over the left ends and one over
 *       the right ends, rows top to bottom, empty rows skipped, collinear points dropped (vertices are strict).
 *       shape[.][5] = hull_area2: twice the polygon's area (shoelace sum, an exact integer; 0 for a point or a line);
 *       shape[.][6] = hull_pts: number of strict vertices -- 1 for a single pixel, 2 for any straight line of pixels;
 *       shape[.][7] = rows: rows of the box with at least one pixel.  All three are 0 for an absent id and -1 for a box side >= 2^16 (not computed).
 *     hull_pts_out: int32 [2 x sum of box heights][2] or NULL (areas only).  The vertices of instance i start at point slot 2 * row_offsets[i], x then
 *       y, at most 2 x box height of them, counter-clockwise on the screen (y down) from the top-left vertex (the leftmost pixel of the top row): down
 *       the left side, along the bottom, up the right side.  Slots past hull_pts are not written.
 *
 * cerb_inst_relate  one thread per child instance i (row i of child_table, a cerb_inst_table of the CHILD map): its integer centroid is
 *       (cx, cy) = (sum_x / area, sum_y / area), floor division; parent_of[i] = parent_labels[cy >> shift][cx >> shift], and 0 when that pixel lies
 *       outside ph x pw, holds an id outside [1, n_parent], or the child is absent (area 0).  parent_of: int32 [n_child].
 *     parent_rows: int64 [n_parent][CERB_INST_PARENT_WORDS], cleared by the call; the row of parent p (row p-1) gains {children, sum of child areas,
 *       children of class 0..7} with class = child_type[i] & 7 (child_type: int32 [n_child] or NULL = the class columns stay 0).
 *     shift is 0 when both maps share a grid and 1 when the child map is at full resolution and the parent map at x0.5.  Child areas are in CHILD-map
 *       pixels whatever the shift.
 *
 * cerb_points_knn  xy: int32 [n][2], coordinates of absolute value < 2^26; 1 <= k <= 8.  idx_out: int32 [n][k], the k nearest OTHER points by exact
 *       int64 squared distance, ascending by (d2, index) -- a tie goes to the smaller index; -1 fills the row where n - 1 < k.  d2_out: int64 [n][k],
 *       -1 beside a -1 index.  Brute force, n^2 distances (candidate tiles staged through LDS, k best per thread in registers): meant for gland and
 *       lumen graphs of 10^3..10^5 points. */
#define CERB_INST_SHAPE_WORDS 8
#define CERB_INST_PARENT_WORDS 10
int cerb_inst_shape(const int32_t* labels, long long lab_row_stride, int h, int w, int n_inst, const long long* table, long long* shape,
                    void* hip_stream);
int cerb_inst_hull_rows(const int32_t* labels, long long lab_row_stride, int h, int w, int n_inst, const long long* table,
                        const long long* row_offsets, int32_t* extents, int32_t* hull_pts_out, long long* shape, void* hip_stream);
int cerb_inst_relate(const long long* child_table, int n_child, const int32_t* child_type, const int32_t* parent_labels,
                     long long parent_row_stride, int ph, int pw, int shift, int n_parent, int32_t* parent_of, long long* parent_rows,
                     void* hip_stream);
int cerb_points_knn(const int32_t* xy, int n, int k, int32_t* idx_out, long long* d2_out, void* hip_stream);

/* ---- training augmentations: the shape and input augmentations in front of gen_targets (loader/augs.py lambdas + affine / flip / crop) --------------
 * The host draws every random number (cerberus_amd/augs.py: sample_params) and uploads a few numbers per sample; every call below is a pure function
 * of (input, per-sample parameter arrays), runs the whole batch in ONE launch on hip_stream, allocates nothing and does not synchronise.  Images are
 * uint8 [n][h][w][3] (RGB), annotations int32 [n][h][w][c], both dense; parameter arrays are device arrays of n entries.  The definitions are this
 * project's own, in integers and float64 (binary64, every product, quotient and sum rounded on its own -- no fused multiply-add): bit parity with
 * OpenCV / imgaug is NOT claimed; where OpenCV documents its 8-bit behaviour (H in 0..179, the sigma = 0 Gaussian tables, the
 * fixed-point grey weights) the definitions follow it, pinned by tests/golden/augs_documented.json.
 * Every call refuses (error, no launch): a null pointer, n outside 1..65535, an empty image, a side above 16384.  The stencil calls (warp, the two
 * blurs) are out of place and refuse overlapping src / dst; the point-wise calls (noise, colour) accept dst == src and refuse any other overlap.
 *
 * cerb_aug_warp: affine + centre crop + flips of image and annotation in one nearest-neighbour gather.
 *   maps: int64 [n][6] = (A, B, C, D, E, F) in Q16.  For the output pixel (u, v) = (column, row), in 64-bit integers with an arithmetic shift:
 *       xs = (A u + B v + C + 32768) >> 16,   ys = (D u + E v + F + 32768) >> 16
 *   out[v][u] = src[ys][xs] (all channels of both arrays) when 0 <= xs < src_w and 0 <= ys < src_h, else 0.  Either array (with its output) may be NULL.
 *   The host composes the map (cerberus_amd/augs.py: compose_map): the forward map in (x, y) pixel coordinates of the src_w x src_h canvas is
 *       M = T(c + t) R(theta) Shear_x(phi) S(sx, sy) T(-c),  c = ((src_w - 1) / 2, (src_h - 1) / 2),
 *       R = [cos -sin; sin cos], Shear_x = [1 tan(phi); 0 1], S = diag(sx, sy), T = translation, multiplied left to right as 3 x 3 float64 matrices;
 *   with M = [a b c; d e f; 0 0 1] and det = a e - b d its inverse is [e/det  -b/det  (b f - c e)/det;  -d/det  a/det  (c d - a f)/det]; each of the six
 *   entries m becomes int(rint(m * 65536)).  Then, exactly in integers: the centre crop to out_h x out_w with (oy, ox) = ((src_h - out_h) / 2,
 *   (src_w - out_w) / 2) (floor): C += A ox + B oy, F += D ox + E oy; a left-right flip of the OUTPUT: C += A (out_w - 1), F += D (out_w - 1), A = -A,
 *   D = -D; an up-down flip: C += B (out_h - 1), F += E (out_h - 1), B = -B, E = -E.
 *
 * cerb_aug_gaussian_blur: per sample (kx[i], ky[i]), each in {1, 3, 5}: weights [1], [1 2 1] (sum 4), [1 4 6 4 1] (sum 16) -- OpenCV's tables for
 *   sigma = 0 --, borders replicate (the coordinate is clamped), out = (sum_y sum_x wy wx p + half) >> shift with shift = log2(sum_x sum_y) and
 *   half = 2^(shift-1) (0 when shift = 0): round half up, in integers.  kx = ky = 1 is a copy.
 * cerb_aug_median_blur: per sample k[i] in {1, 3, 5}: per channel the median (element k k / 2 of the sorted k x k window), borders replicate.
 *   For both blurs a size of 0 (or any value outside {1, 3, 5}) leaves that sample of dst UNWRITTEN: augment_batch runs the blur, the median and the
 *   noise call on the same src / dst pair and each sample is written by exactly one of them.
 *
 * cerb_aug_gaussian_noise: per sample sigma[i] (float64), per_channel[i] (int32, 0 / non-zero), key[i] (uint64).  For pixel index q = v w + u of the
 *   sample, Philox4x32-10 (Salmon et al. 2011; multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85) with key (key & 0xffffffff, key >> 32) and
 *   counter (q & 0xffffffff, q >> 32, 0, 0) gives r0..r3;  u1 = (r0 + 1) 2^-32, u2 = r1 2^-32, u3 = (r2 + 1) 2^-32, u4 = r3 2^-32;
 *   z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = sqrt(-2 ln u1) sin(2 pi u2), z2 = sqrt(-2 ln u3) cos(2 pi u4), with 2 pi = 6.283185307179586.
 *   per_channel: channels (R, G, B) get (z0, z1, z2); otherwise all three get z0.  out = clip(floor(p + sigma z + 0.5), 0, 255) in float64.
 *   sigma = 0 is a copy.  A sigma that is not finite leaves that sample of dst UNWRITTEN.  (ln / cos / sin come from the device's math library:
 *   a result may differ from another library's where p + sigma z + 0.5 lies within rounding of an integer -- tests/test_augs_gpu.py states the rule.)
 *
 * Colour, one call per operation, value[i] float64 per sample; a value that is not finite SKIPS the sample (copied when dst != src).  p = a channel
 * value, trunc(clip(x, 0, 255)) = the float64 -> uint8 store of numpy after np.clip:
 *   cerb_aug_brightness  out = trunc(clip(p + value, 0, 255)).
 *   cerb_aug_saturation  g = (4899 R + 9617 G + 1868 B + 8192) >> 14 (OpenCV's 8-bit grey), s = 1 + value, out = trunc(clip(p s + g (1 - s), 0, 255)).
 *   cerb_aug_hue         RGB -> HSV in integers: V = max, d = V - min, S = floor((510 d + V) / (2 V)) (round-half-up of 255 d / V; 0 when V = 0);
 *                        H = 0 when d = 0, else with hnum = G - B if V = R, else (B - R) + 2 d if V = G, else (R - G) + 4 d:
 *                        H = floor((60 hnum + d) / (2 d)), plus 180 if negative, minus 180 if >= 180 (H in 0..179).
 *                        Shift: x = H + value; r = fmod(x, 180), plus 180 if r < 0 (the divisor's sign, as numpy's %); H' = trunc(r).
 *                        HSV -> RGB: s = S / 255, v = V, hh = H' / 30, i = floor(hh), f = hh - i, p = v (1 - s), q = v (1 - s f), t = v (1 - s (1 - f));
 *                        (R, G, B) = (v,t,p), (q,v,p), (p,v,t), (p,q,v), (t,p,v), (v,p,q) for i mod 6 = 0..5; each rounded half to even to uint8.
 *   cerb_aug_contrast    mean_c = sums[i][c] / (h w) in float64 (sums: int64 [n][3] from cerb_aug_channel_sums of the same src);
 *                        out = trunc(clip(p value + mean_c (1 - value), 0, 255)).  The reference's add_to_contrast returns its INPUT
 *                        (loader/augs.py:71-78 clips `img`, not `ret`): cerberus_amd.augs mirrors that by default and calls this only on request.
 *   cerb_aug_channel_sums  sums[i][c] = the exact integer sum of channel c of sample i (the call clears sums; integer partial sums, 64-bit integer atomics). */
int cerb_aug_warp(const uint8_t* img, const int32_t* ann, int n, int src_h, int src_w, int ann_c, const int64_t* maps, uint8_t* img_out,
                  int32_t* ann_out, int out_h, int out_w, void* hip_stream);
int cerb_aug_gaussian_blur(const uint8_t* src, uint8_t* dst, int n, int h, int w, const int32_t* kx, const int32_t* ky, void* hip_stream);
int cerb_aug_median_blur(const uint8_t* src, uint8_t* dst, int n, int h, int w, const int32_t* k, void* hip_stream);
int cerb_aug_gaussian_noise(const uint8_t* src, uint8_t* dst, int n, int h, int w, const double* sigma, const int32_t* per_channel,
                            const uint64_t* key, void* hip_stream);
int cerb_aug_brightness(const uint8_t* src, uint8_t* dst, int n, int h, int w, const double* value, void* hip_stream);
int cerb_aug_saturation(const uint8_t* src, uint8_t* dst, int n, int h, int w, const double* value, void* hip_stream);
int cerb_aug_hue(const uint8_t* src, uint8_t* dst, int n, int h, int w, const double* value, void* hip_stream);
int cerb_aug_contrast(const uint8_t* src, uint8_t* dst, int n, int h, int w, const double* value, const int64_t* sums, void* hip_stream);
int cerb_aug_channel_sums(const uint8_t* src, int n, int h, int w, int64_t* sums, void* hip_stream);

/* ---- instance overlays: closed contours drawn over a picture (misc/viz_utils.py:150-214; cerberus_amd/viz.py) ---------------------------------------
 * The project's own definition, in integers throughout: cv2.drawContours is not pinned.  Three calls on hip_stream, none of which
 * allocates or synchronises: clear the priority plane, stamp groups of contours into it, resolve it into the picture.
 *
 * Covered pixel.  A pixel (x, y) is covered by the segment a -> b drawn with width w (1..255) iff the distance from its centre to the segment is at
 * most w / 2.  With v = b - a, u = p - a, vv = v.v, t = u.v, c = ux vy - uy vx (int64):
 *     vv == 0 or t <= 0 :  covered iff 4 (u.u) <= w^2
 *     t >= vv           :  covered iff 4 |p - b|^2 <= w^2
 *     otherwise         :  covered iff |c| <= isqrt(floor(w^2 vv / 4)),   isqrt = the exact integer square root
 *   A round-capped, round-jointed stroke.  A zero-length segment is a disk: 1 pixel for w = 1, the 5-pixel plus for w = 2, the full 3 x 3 for w = 3.
 *   An EVEN width paints w + 1 pixels across an axis-aligned line (the integers with |c| <= w / 2), an odd width w.
 * Contours.  Contour i has counts[i] points, points[offsets[i] .. offsets[i] + counts[i]) (int32 (x, y) pairs), and is closed: segment k runs from
 *   point k to point (k + 1) mod count.  A count of 0 (or below) draws nothing, 1 a disk, 2 one capsule.  Offsets need not be contiguous or ordered.
 * Point transform, per call, in int64: q = p mul - (org_x, org_y), p' = q / div truncated toward zero (C division; numpy's astype("int") of the
 *   quotient).  mul in 1..16, div in 1..4096, |org| <= 2^40.  A contour with ANY transformed coordinate outside [-2^20, 2^20] is skipped as a whole.
 *   Every segment's box is expanded by (w + 1) / 2 and clipped to the image: no loop is longer than the image.
 * Painter's order.  The workspace is a plane of uint32, one per output pixel: the largest ORDINAL of the contours covering the pixel, 0 = none, written
 *   with an integer atomic max -- the result does not depend on the execution order.  Contour i of a stamp call has ordinal first_ordinal + i + 1
 *   (contours with no points keep theirs): first_ordinal = the number of contours stamped since the clear, so that groups with different widths share
 *   one plane and a later contour overwrites an earlier one.  first_ordinal + n must stay below 2^32 - 1.
 * Resolve.  dst[y][x] = colours[prio - 1] where prio = plane[y][x] is in 1..n_total, and src[y / up][x / up] elsewhere: the nearest-neighbour
 *   up-scaling (up in 1..8, out_h == src_h up, out_w == src_w up) is part of the pass.  Both images are uint8 RGB with row strides in bytes (bytes
 *   between rows are not touched); a colour is the uint32 word R | G << 8 | B << 16.  dst must not overlap src.
 * Refusals (an error, no launch, nothing written): a null pointer (colours may be NULL when n_total is 0), a side outside 1..32768, width / mul / div /
 *   up out of range, a workspace smaller than cerb_overlay_workspace_bytes(out_h, out_w) = 4 out_h out_w (0 for a refused size) or not 4-byte aligned,
 *   a negative n, a row stride shorter than its row. */
size_t cerb_overlay_workspace_bytes(int out_h, int out_w);
int cerb_overlay_clear(void* ws, size_t ws_bytes, int out_h, int out_w, void* hip_stream);
int cerb_overlay_stamp(const int32_t* points, const int64_t* offsets, const int32_t* counts, long long n, int mul, int div, long long org_x,
                       long long org_y, int width, long long first_ordinal, void* ws, size_t ws_bytes, int out_h, int out_w, void* hip_stream);
int cerb_overlay_resolve(const uint8_t* src, long long src_row_stride, int src_h, int src_w, int up, const uint32_t* colours, long long n_total,
                         const void* ws, size_t ws_bytes, uint8_t* dst, long long dst_row_stride, int out_h, int out_w, void* hip_stream);

/* ---- label maps from contours: polygon fill into the overlay's plane (cerberus_amd/rasterize.py) ---------------------------------
 * The step back from an instance dictionary (closed contours) to an int32 label map.  The project's own definition, in integers throughout:
 * cv2.drawContours(thickness=FILLED) / fillPoly are not pinned.  Contours, point transform, the skip rule (a contour with any transformed
 * coordinate outside [-2^20, 2^20] is skipped as a whole -- fill and outline never disagree about which contours exist), plane, ordinals and limits are
 * the stamp's, above.
 *
 * Interior.  Pixel (x, y) is interior to a contour of at least 3 points iff an ODD number of its edges a -> b satisfy both
 *     min(ay, by) <= y < max(ay, by)                     (half-open: a horizontal edge never counts, a vertex on a pixel row counts once)
 *     xc <= x,  xc = ax + ceil((y - ay) (bx - ax) / (by - ay))     (the exact integer ceiling, in int64)
 *   -- the even-odd rule on pixel centres with the ray pointing left; a self-intersecting polygon follows even-odd.  Contours with fewer than 3 points
 *   have no interior.  cerb_overlay_fill paints the interior alone.
 * Filled set = interior + the width-1 stroke of the same contour: cerb_overlay_fill and cerb_overlay_stamp(width = 1) with the same first_ordinal, in
 *   either order.  Because the outline always belongs to the set, the tie rule for pixels exactly on an edge (xc <= x and not xc < x) does not matter:
 *   such a pixel lies within 1 / 2 of the edge and the stroke covers it.  For a contour made of 8-direction runs (everything cerb_inst_contour_points
 *   emits) the width-1 stroke is exactly the contour's lattice points, and the filled set of the outer contour of an instance that is one 8-connected
 *   piece without holes is the instance itself: a dictionary rasterises back to the label map it came from.  Holes (interior rings) do not exist here.
 * Painter's order.  As the stamp: a filled pixel takes max(plane, ordinal), ordinal = first_ordinal + i + 1.
 * Labels.  dst[y][x] = table[prio - 1] where prio = plane[y][x] is in 1..n_total, and `background` elsewhere; table is int32 [n_total] and several
 *   contours may carry one value (the rings of a MultiPolygon; the instances' types for a class map).  dst is int32 with its row stride in BYTES, a
 *   multiple of 4 (bytes between rows are not touched).
 * Neither call allocates or synchronises.  Refusals (an error, no launch, nothing written): a null pointer (table may be NULL when n_total is 0) or one
 *   that is not 4-byte aligned, a side outside 1..32768, mul / div out of range, a workspace smaller than cerb_overlay_workspace_bytes or not 4-byte
 *   aligned, a negative n or n_total, first_ordinal + n >= 2^32 - 1, a row stride shorter than its row or no multiple of 4. */
int cerb_overlay_fill(const int32_t* points, const int64_t* offsets, const int32_t* counts, long long n, int mul, int div, long long org_x,
                      long long org_y, long long first_ordinal, void* ws, size_t ws_bytes, int out_h, int out_w, void* hip_stream);
int cerb_overlay_labels(const int32_t* table, long long n_total, int background, const void* ws, size_t ws_bytes, int32_t* dst,
                        long long dst_row_stride, int out_h, int out_w, void* hip_stream);

int cerb_event_create(void** ev);
int cerb_event_record(void* ev, void* hip_stream);
int cerb_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms); /* synchronises on ev_stop */
int cerb_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* CERBERUS_HIP_H */
