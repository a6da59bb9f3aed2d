"""nsof -- MI355X-native neuromorphic optical-flow core (host-side Python mirror).

Mirrors the two interfaces the reference's scripts call on the hot path:

* ``calcOpticalFlowFarneback(prev, next, flow, pyr_scale, levels, winsize, iterations,
  poly_n, poly_sigma, flags)`` -- same positional order and keyword names as
  ``cv2.calcOpticalFlowFarneback`` at /root/reference/optical_flow_seg.py:203
  (``farneback_params`` dict at :73-81); ``install()`` assigns it onto ``cv2`` so the
  reference's seg/ob/prediction scripts run unmodified where cv2 exists.
* ``simulate(...)``, ``update_state(w, V, p, dt)``, ``resistance_exp(w, p)`` -- the accumulator of
  /root/reference/eventsim/event_mem_sim.py:40-63,164-286.

All arithmetic runs in libnsof.so (HIP, gfx950).  No fallbacks.
"""
from .errors import NsofError, error  # noqa: F401
from .context import Context, default_context  # noqa: F401
from .farneback import (OPTFLOW_FARNEBACK_GAUSSIAN, OPTFLOW_USE_INITIAL_FLOW, FarnebackParams, StreamPool, calcOpticalFlowFarneback, effective_levels, farneback_batch,  # noqa: F401
                        farneback_many, farneback_pairs, farneback_pairs_16_dev, farneback_pairs_dev,
                        farneback_pairs_f32_dev, farneback_roi_sequence_16_dev, farneback_roi_sequence_dev,
                        farneback_roi_sequence_f32_dev,
                        farneback_sequence, install, level_size,
                        pinned_empty, uninstall)
from .accumulator import (PARAMS, DT, THETA_EVENTS, REFRACTORY_US, Accumulator, TrialAccumulator, accum_params, bincount_2d,  # noqa: F401
                          c2c_arg, c2c_noise, frame_param_maps_arg, generate_synthetic_events, load_events, resistance_exp, simulate, simulate_frames, simulate_frames_dev,
                          simulate_trials, simulate_trials_dev, slice_indices, trial_param_maps_arg, update_state, variability_maps)

from .gating import (GatingConfig, connectedComponentsWithStats, current_to_gray, dataset_config, frame_to_gray,  # noqa: F401,E402
                     gate_stats, gate_stats_dev, gating_maps, load_gating_stack, opticalFlow3D, process_merged_region, process_separate_regions, update_transition_pic)
from .segment import (MORPH_CROSS, MORPH_ELLIPSE, MORPH_RECT, dilate, erode, getStructuringElement, motion_mask,  # noqa: F401,E402
                      motion_mask_dev, motion_mask_sequence_dev, pixel_accuracy_batch_dev, process_flow_region,
                      task_results)
from .predict import (BORDER_CONSTANT, BORDER_REPLICATE, INTER_LINEAR, calculateIntegralError, gray_u8_dev,  # noqa: F401,E402
                      predict_region, predict_region_dev, predict_sequence_dev, remap, ssim_batch_dev,
                      structural_similarity)
from .pipeline import events_variability_dev, gating_stack_from_frames_dev, gating_variability_dev, prediction_sequence_dev, run_prediction, run_segmentation, segmentation_sequence_dev  # noqa: F401,E402
from .frames import compress_image, crop_image, im2double, imresize_lanczos3, process_images, process_images_dev  # noqa: F401,E402
from .flowviz import flow_to_image, flow_to_image_dev, flow_uv_to_colors, make_colorwheel, save_viz, viz  # noqa: F401,E402
from .flowstats import events_flow_variability_dev, flow_ensemble_dev, flow_ensemble_summary  # noqa: F401,E402
from .events import events_from_frames_dev, events_from_video_dev, events_noise_draw, linear_response, log_response, render_box_frames  # noqa: F401,E402
from .denoise import events_denoise_dev  # noqa: F401,E402

__all__ = ["calcOpticalFlowFarneback", "install", "uninstall", "FarnebackParams", "farneback_batch", "Context",
           "default_context", "simulate", "update_state", "resistance_exp", "Accumulator", "NsofError", "error"]
