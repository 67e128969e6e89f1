"""Command lines of the two inference drivers.  The reference parses docopt usage strings (run_infer_tile.py, run_infer_wsi.py);
docopt is not installed here and the drivers behind the flags are different programs, so the interface is a table: flag NAMES and
DEFAULTS are the reference's (a maintainer's existing command lines keep working, `--flag=value` or `--flag value`), the help
text and everything behind it are this package's."""
import sys

# (flag, takes a value, default, help)
_COMMON = [
    ("--gpu", True, "0", "GPU id(s), exported as HIP_VISIBLE_DEVICES when not launched under torch.distributed.run; several ids (`0,1,2`) = one rank per "
                          "device, self-spawned (cerberus_amd/launch.py): slide bands / the tile file list are sharded over them"),
    ("--model", True, None, "directory holding settings.yml + weights.tar (required unless --synthetic)"),
    ("--synthetic", False, False, "(not in the reference) run on the package's seeded synthetic test weights instead of a checkpoint"),
    ("--nr_inference_workers", True, "0", "accepted for compatibility: tiles are gathered on the device, there is no loader pool"),
    ("--nr_post_proc_workers", True, "0", "accepted for compatibility: post-processing runs on the GPU in the main process"),
]
TILE_OPTIONS = _COMMON + [
    ("--batch_size", True, "10", "tiles per forward"),
    ("--input_dir", True, None, "directory of .png / .jpg tiles (searched recursively)"),
    ("--output_dir", True, "output/", "where <tissue>_mat/, pclass_mat/ and overlay/ are written"),
    ("--patch_input_shape", True, "448", "network input window (square)"),
    ("--patch_output_shape", True, "144", "centre crop kept from every window (square)"),
    ("--overlay", True, "host", "(not in the reference) host | device: where overlay/<name>.jpg is drawn -- host: PIL on the writer threads, contour by contour; "
                                "device: the contour rasteriser (cerb_overlay_*, cerberus_amd/viz.py) with the x2 up-scaling fused, the writer threads only "
                                "encode the JPEG.  The two strokes differ in a cosmetic share of the painted pixels; the .mat files are the same"),
    ("--overlay_encode", True, "host", "(not in the reference) host | device: where overlay/<name>.jpg is JPEG-encoded -- host: PIL on the writer threads; device: with "
                                       "--overlay=device only, the picture never leaves the device: colour conversion, DCT, Huffman coding and packing run in HIP "
                                       "(cerb_jpeg_enc_*, cerberus_amd/jpeg_encode.py) and the writer threads receive the compressed bytes.  The same pixels "
                                       "on decoding; the file has one restart interval per MCU row"),
]
WSI_OPTIONS = _COMMON + [
    ("--batch_size", True, "30", "patches per forward"),
    ("--tile_shape", True, "2048", "accepted and ignored (the reference overrides it too): maps stay in HBM, nothing is tiled"),
    ("--chunk_shape", True, "15000", "accepted and ignored"),
    ("--ambiguous_size", True, "64", "accepted and ignored: bands are labelled in one pass, seams are exact (shard_postproc)"),
    ("--wsi_proc_mag", True, "0.5", "microns per pixel recorded in the instance dictionary"),
    ("--wsi_file_ext", True, ".svs", "slide extension: .npy arrays, .png/.jpg images or .txt `synthetic:<H>x<W>:<seed>` specs"),
    ("--cache_path", True, "cache/", "accepted and ignored: there is no memmap cache"),
    ("--logging_dir", True, "logging/", "one <slide>_<date>_std.log per slide and run with its phase timings (rank 0)"),
    ("--input_dir", True, None, "directory of slides (not searched recursively)"),
    ("--msk_dir", True, None, "directory of tissue masks <slide>.png (any resolution); when given, only slides that have a mask are processed"),
    ("--output_dir", True, "output/", "where dat/<slide>.dat, tissue/<slide>.mat (and <slide>.npz with --save_label_maps) are written"),
    ("--patch_input_shape", True, "448", "network input window (square)"),
    ("--patch_output_shape", True, "144", "centre crop kept from every window (square)"),
    ("--wsi_bulk_idx", True, "1", "accepted for compatibility"),
    ("--wsi_proc_step", True, "10", "accepted for compatibility"),
    ("--save_thumb", False, False, "accepted and ignored"),
    ("--save_mask", False, False, "write the tissue mask used as <output_dir>/mask/<slide>.png"),
    ("--save_label_maps", False, False, "(not in the reference) also dump the label / class maps as <output_dir>/<slide>.npz"),
    ("--reference_tiling", False, False, "(not in the reference) nuclei instances through the reference's own 4096 x 4096 tiles, 64-px margins, strips and "
                                         "cross sections (infer/wsi.py:81-268, 642-684; cerberus_amd/ref_tiling.py) instead of exact band ownership: the "
                                         "reference's instance set, including the few seam instances its scheme drops; tiles are sharded over the ranks"),
    ("--jpeg_decode", True, "host", "(not in the reference) host | device: where the JPEG tiles of .svs / tiled TIFF slides are decoded -- host: PIL / libjpeg, tile by "
                                    "tile (unless CERB_JPEG_DECODE says otherwise); device: native Huffman pass on the host, inverse DCT / up-sampling / colour in HIP "
                                    "kernels, the same bytes (sets CERB_JPEG_DECODE=device; cerberus_amd/jpeg_device.py)"),
    ("--auto_mask", False, False, "(not in the reference's command line) generate the tissue mask of every slide on the device from a thumbnail -- the reference's "
                                  "get_tissue_mask (misc/utils.py:195-244; cerberus_amd/tissue.py) -- and use it like a --msk_dir mask; not together with --msk_dir"),
    ("--auto_mask_ds", True, "16", "(not in the reference) with --auto_mask: the thumbnail is the slide at 1/<n> of the processing resolution"),
]
# WSI_OPTIONS is pinned, entry by entry, by tests/test_tissue_mask_host.py and is closed: every NEW run_infer_wsi.py option goes into WSI_MODEL_OPTIONS
# below (appended at its end) or into WSI_OUTPUT_OPTIONS further down, and run_infer_wsi.py parses all three tables (WSI_DRIVER_OPTIONS).
WSI_MODEL_OPTIONS = [
    ("--eroded_maps", False, False, "(not in the reference's command line) run a model whose INST heads carry the IP-ERODED-3 / -11 codes (two classes, PostProcInstErodedMap) "
                                    "on slides: one-channel canvases, the eroded labelling inside the band / halo / ownership protocol; without the flag such a "
                                    "model is refused by name.  Not with --reference_tiling when the Nuclei head is such a head; slides that would need sub-band "
                                    "streaming are refused"),
]
WSI_ALL_OPTIONS = WSI_OPTIONS + WSI_MODEL_OPTIONS
# WSI_ALL_OPTIONS is pinned as well (tests/test_eroded_wsi_host.py): options about what the driver WRITES go here, and run_infer_wsi.py parses
# WSI_DRIVER_OPTIONS = WSI_ALL_OPTIONS + WSI_OUTPUT_OPTIONS.
WSI_OUTPUT_OPTIONS = [
    ("--save_overlay", False, False, "(not in the reference) write <output_dir>/overlay/<slide>.jpg: the slide at 1/--overlay_ds of the processing resolution with every "
                                     "instance of dat/<slide>.dat drawn on it on the device (line width 2; the reference's visualize_instances_dict, "
                                     "misc/viz_utils.py:150-184); needs a slide with a reader (not a `synthetic:` spec)"),
    ("--overlay_ds", True, "8", "(not in the reference) with --save_overlay: the picture is the slide at 1/<n> of the processing resolution, n a whole number >= 1; "
                                "a picture side above 32768 is refused"),
    ("--overlay_encode", True, "host", "(not in the reference) host | device, with --save_overlay only: where overlay/<slide>.jpg is JPEG-encoded -- host: the picture is "
                                       "downloaded and PIL encodes it; device: it is encoded in HIP (cerb_jpeg_enc_*, cerberus_amd/jpeg_encode.py) and only the "
                                       "compressed bytes are downloaded.  The same pixels on decoding; the file has one restart interval per MCU row"),
    ("--save_overlay_tiff", False, False, "(not in the reference) write <output_dir>/overlay/<slide>.tif: the slide at the FULL processing resolution with every instance of "
                                          "dat/<slide>.dat drawn on it (half the tile overlay's line widths), as a pyramidal JPEG-tiled BigTIFF that QuPath, ASAP and "
                                          "OpenSlide open; drawn, reduced and JPEG-encoded on the device window by window (cerberus_amd/tiff_pyramid.py, "
                                          "viz.slide_overlay_pyramid).  Independent of --save_overlay, --overlay_ds and --overlay_encode; needs a slide with a reader "
                                          "(not a `synthetic:` spec)"),
]


def check_overlay_encode(args, drawn_on_device, needs):
    """--overlay_encode=device encodes a picture that is already on the device: refused by name where there is none (ValueError naming both options)."""
    if args["--overlay_encode"] not in ("host", "device"):
        raise ValueError("--overlay_encode takes host or device, got %r" % (args["--overlay_encode"],))
    if args["--overlay_encode"] == "device" and not drawn_on_device:
        raise ValueError("--overlay_encode=device needs %s: the encoder takes the picture the device drew, and without it there is none" % needs)
WSI_DRIVER_OPTIONS = WSI_ALL_OPTIONS + WSI_OUTPUT_OPTIONS
# compute_stats.py (not a driver of the reference's command line: its compute_stats.py is a script with paths edited in place)
STATS_OPTIONS = [
    ("--gpu", True, "0", "GPU id, exported as HIP_VISIBLE_DEVICES"),
    ("--pred_dir", True, None, "the --output_dir of run_infer_tile.py: <pred_dir>/<tissue>_mat/<name>.mat are read ('inst_map', and 'id' / 'type' with --types); "
                               "stats.csv is written here"),
    ("--true_dir", True, None, "directory of <name>.mat or <name>.npy annotations holding 'inst_map' and optionally 'inst_type' (one class per instance, in "
                               "ascending id order)"),
    ("--tissue", True, "nuclei", "which <tissue>_mat to score: nuclei | gland | lumen"),
    ("--types", True, None, "number of classes, background included: also report PQ per class 1 .. n-1 and their mean (needs 'inst_type' on the true side)"),
    ("--pred_dat", True, None, "instead of --pred_dir / --true_dir: the dat/<slide>.dat of run_infer_wsi.py; its contours are filled into a label map on the device "
                               "(cerberus_amd/rasterize.py) and scored against --true_ann; classes for --types are the instances' 'type' entries; "
                               "<slide>_stats.csv is written beside the file"),
    ("--true_ann", True, None, "with --pred_dat: the annotation -- another .dat, a .json of the reference's save_json, a .geojson FeatureCollection (QuPath's "
                               "export; polygons without holes) or a label-map .npz (keys Nuclei / Gland / Lumen, type_* class maps for --types)"),
]

# compute_features.py (not in the reference: its misc/viz_utils.py visualize_graph sketches the gland graph these tables feed)
FEATURES_OPTIONS = [
    ("--gpu", True, "0", "GPU id, exported as HIP_VISIBLE_DEVICES"),
    ("--pred_dir", True, None, "the --output_dir of run_infer_tile.py: <pred_dir>/{nuclei,gland,lumen}_mat/<name>.mat are read ('inst_map', 'id', 'type'); "
                               "<pred_dir>/features/<name>_{nuclei,gland,lumen}.csv are written"),
    ("--npz", True, None, "a <slide>.npz of run_infer_wsi.py --save_label_maps (keys Nuclei, Gland, Lumen, type_*): gland and lumen maps at the nuclei "
                          "map's resolution or at half of it; the CSVs are written to <directory of the file>/features/"),
    ("--knn", True, "4", "neighbours per gland in the gland table (1 .. 8; 0: none)"),
    ("--dat", True, None, "a dat/<slide>.dat of run_infer_wsi.py: the label maps are filled from its contours on the device (cerberus_amd/rasterize.py), gland "
                          "and lumen at half the resolution as the slide driver keeps them; the same CSVs as --npz, written to <directory of the file>/features/"),
]


def usage(prog, options):
    lines = ["usage: %s [options]" % prog, "", "options:", "  -h, --help", "  --version"]
    for flag, has_val, default, text in options:
        left = flag + ("=<value>" if has_val else "")
        lines.append("  %-30s %s%s" % (left, text, "" if default in (None, False) else "  [default: %s]" % default))
    return "\n".join(lines)


def require_model(args):
    """A forgotten --model must not produce plausible-looking label maps from synthetic weights."""
    if not args.get("--model") and not args.get("--synthetic"):
        sys.exit("--model=<dir with settings.yml + weights.tar> is required (or --synthetic for the seeded test weights)")


def parse(prog, options, argv=None, version=None):
    """Returns {flag: value}: strings for valued flags (None when absent and without default), booleans for switches."""
    argv = list(sys.argv[1:] if argv is None else argv)
    opts = {flag: default for flag, _, default, _ in options}
    valued = {flag: has_val for flag, has_val, _, _ in options}
    if "-h" in argv or "--help" in argv:
        print(usage(prog, options))
        sys.exit(0)
    if "--version" in argv:
        print(version)
        sys.exit(0)
    i = 0
    while i < len(argv):
        key, eq, val = argv[i].partition("=")
        if key not in opts:
            print(usage(prog, options))
            sys.exit("unknown option %s" % argv[i])
        if not valued[key]:
            opts[key] = True
        elif eq:
            opts[key] = val
        else:
            i += 1
            if i >= len(argv):
                sys.exit("option %s needs a value" % key)
            opts[key] = argv[i]
        i += 1
    return opts
