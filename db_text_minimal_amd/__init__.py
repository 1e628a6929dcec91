"""db_text_minimal_amd — MI355X-native DBNet hot path (model forward/backward,
DBLoss, per-step update) behind the call surface of huyhoang17/DB_text_minimal."""
from .losses import DBLoss  # noqa: F401
from .models import DBTextModel  # noqa: F401
from .optim import FusedAdam, FusedAdamW, FusedSGD, split_decay  # noqa: F401
from .lr_schedulers import WarmupPolyLR  # noqa: F401
from .train import DBTrainer  # noqa: F401
from .gt_maps import gt_collate, make_gt_maps, normalize_images, offset_polygon  # noqa: F401
from .postprocess import SegDetectorRepresenter, detect_boxes, detect_polygons  # noqa: F401
from .det_eval import DetectionDetEvalEvaluator, DetectionIoUEvaluator, QuadMetric, polygon_overlaps  # noqa: F401
from .augment import DeviceBatches, augment_images, image_collate, plan_augment, plan_letterbox, preprocess_image  # noqa: F401
from .photometric import (adjust_brightness, adjust_contrast, adjust_hue, adjust_saturation, color_jitter_images,  # noqa: F401
                          plan_color_jitter)
from .degrade import blur_weights, degrade_images, degrade_records, gaussian_blur, gaussian_noise, plan_degrade  # noqa: F401
from .synth import SynthTextBatches, plan_synth_text, render_synth_text, synth_records  # noqa: F401
from .word_crops import (crop_words, perspective_maps, polygon_ribbons, polygon_ribbons_device, rectify_from_ribbons,  # noqa: F401
                         rectify_words)
from .render import draw_outlines, image_views, minmax_scale_u8, overlay_heatmap, render_detections  # noqa: F401
from .render import draw_dots, draw_labels, draw_scores, draw_words, text_size  # noqa: F401
from .recognise import AttnLabelConverter, CTCLabelConverter, greedy_decode, recognize_words, words_to_input  # noqa: F401
from .spotting import Lexicon, TextClasses, TextSpottingEvaluator, edit_distances  # noqa: F401
from .jpeg import (CorruptJpeg, JpegCoefficients, JpegEncodeError, JpegError, JpegStreams, UnsupportedJpeg, decode_coefficients, decode_jpeg,  # noqa: F401
                   decode_jpeg_batch, encode_jpeg, encode_jpeg_batch, entropy_decode, entropy_encode, entropy_encode_device, forward_coefficients, jpeg_collate,
                   jpeg_info, jpeg_multiscan_collate, optimal_huffman_table, quant_tables, save_jpegs, entropy_decode_device, jpeg_stream_collate, parse_streams)
from .png import (CorruptPng, PngError, PngScanlines, UnsupportedPng, decode_image_batch, decode_png, decode_png_batch, encode_png,  # noqa: F401
                  encode_png_batch, filter_png_rows, inflate_png, png_collate, png_info, save_pngs, unfilter_png)
