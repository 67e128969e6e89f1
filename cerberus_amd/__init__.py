"""cerberus_amd -- MI355X (gfx950) native tiled-inference hot path of Cerberus behind the reference's own API.

Host mirrors of the reference interface (same names / argument meaning):
  cerberus_amd.net_desc.create_model / NetDesc      <- reference models/net_desc.py
  cerberus_amd.run_desc.infer_step                  <- reference models/run_desc.py:439-502
  cerberus_amd.postproc.PostProcInstErodedContourMap <- reference loader/postproc.py:268-407
  cerberus_amd.tile / cerberus_amd.wsi              <- reference infer/tile.py, infer/wsi.py (geometry + stitching)
  cerberus_amd.targets.gen_targets (+ _batch)       <- reference loader/targets.py:185-244 with loader/augs.py fix_mirror_padding
  cerberus_amd.valid_stats.ValidStats / valid_step_stats / validate <- reference models/run_desc.py:606-747 (ProcStepRawOutput) and :505-565
  cerberus_amd.augs.sample_params / augment_batch / train_batch <- reference loader/augs.py (the lambdas) and the affine / flip / crop steps around them
  cerberus_amd.viz.draw_contours_device / overlay_from_parts / visualize_instances_dict_device <- reference misc/viz_utils.py:150-214 (the overlays)
  cerberus_amd.rasterize.fill_contours_device / label_maps_from_dict / load_annotations <- (not in the reference) label maps back from contours
All arithmetic runs in libcerberus_hip.so (include/cerberus_hip.h); there is no CPU fallback.
"""
__version__ = "0.1.0"


def __getattr__(name):  # cerberus_amd.ValidStats / valid_step_stats / validate / sample_params / ..., imported on first use (the package import stays torch-free)
    if name in ("ValidStats", "valid_step_stats", "validate"):
        from . import valid_stats

        return getattr(valid_stats, name)
    if name in ("sample_params", "augment_batch", "train_batch", "TRAIN_POLICY"):
        from . import augs

        return getattr(augs, name)
    if name in ("draw_contours_device", "contour_colours", "overlay_from_parts", "visualize_instances_dict_device"):
        from . import viz

        return getattr(viz, name)
    if name in ("fill_contours_device", "label_maps_from_parts", "label_maps_from_dict", "load_annotations"):
        from . import rasterize

        return getattr(rasterize, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
